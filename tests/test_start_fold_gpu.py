"""WN.start folded into the first gate GEMM of every flow on the GPU: the window planes and the composed
weight block against their definitions, then WN.forward, forward() and infer() with the fold on against T2S_START_FOLD=0, the CPU
oracle and the golden vectors - at the bars tests/test_waveglow_gpu.py, test_submodules_gpu.py and test_edge_cases_gpu.py apply to
the unfolded path."""
import os

import numpy as np
import pytest
import torch

from text2speech_amd import _lib, planes, synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


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


def _gate_row(o, C):
    """packed row of output channel o of a 2C-row gate convolution (T2S_PERM_GATE, csrc/waveglow_ops.hip pack_dst_row)"""
    gate = int(o >= C)
    ch = o - C if gate else o
    return (ch >> 7) * 256 + ((ch >> 6) & 1) * 128 + (((ch >> 4) & 3) * 2 + gate) * 16 + (ch & 15)


def _set_cols(s, ncol, nwc):
    """first column, counted over the nwc chunks side by side, of column set s (include/t2s_hip.h)"""
    spc = 4 // nwc
    return (s // spc) * 32 + (s % spc) * ncol


@pytest.mark.parametrize("B,nh,c_off,L,taps", [(2, 4, 0, 300, 3), (1, 3, 2, 2051, 3), (3, 2, 4, 64, 3), (1, 4, 0, 5, 5), (2, 1, 6, 1, 3)])
def test_window_planes_match_their_definition(B, nh, c_off, L, taps):
    """(a) t2s_wg_start_window: the window planes are bit-for-bit the four column sets (planes.start_fold_sets) of
    planes.start_window(z[:, c_off:c_off+nh], taps) - the taps of the audio channels and of the ones-channel, zero outside [0, L) -
    the rows outside [0, L) and the unused columns stay zero, and the X planes are what t2s_wg_start writes.  taps = 5 with
    n_half = 4 (25 columns) takes four window chunks, the others two."""
    _lib.load()
    G, C, halo = 8, 128, 128
    ncol = taps * (nh + 1)
    nwc = 2 if 2 * ncol <= 32 else 4
    gen = torch.Generator().manual_seed(L + nh)
    z = torch.randn(B, G, L, generator=gen).to(DEV)
    ws = torch.randn(C, nh, generator=gen).to(DEV)
    bs = torch.randn(C, generator=gen).to(DEV)
    Lp = _lib.plane_rows(L, halo)
    bf = dict(dtype=torch.bfloat16, device=DEV)
    Xh, Xl, Wh, Wl = (torch.zeros(B, C // 32, Lp, 32, **bf), torch.zeros(B, C // 32, Lp, 32, **bf),
                      torch.zeros(B, nwc, Lp, 32, **bf), torch.zeros(B, nwc, Lp, 32, **bf))
    Xh0, Xl0 = torch.zeros_like(Xh), torch.zeros_like(Xl)
    st = _lib.current_stream()
    _lib.call("t2s_wg_start_window", _lib.ptr(z), _lib.ptr(ws), _lib.ptr(bs), B, G, c_off, nh, C, L, Lp, halo, _lib.ptr(Xh),
              _lib.ptr(Xl), taps, nwc, _lib.ptr(Wh), _lib.ptr(Wl), st)
    _lib.call("t2s_wg_start", _lib.ptr(z), _lib.ptr(ws), _lib.ptr(bs), B, G, c_off, nh, C, L, Lp, halo, _lib.ptr(Xh0),
              _lib.ptr(Xl0), st)
    torch.cuda.synchronize()
    assert torch.equal(Xh, Xh0) and torch.equal(Xl, Xl0)
    win = planes.start_window(z[:, c_off:c_off + nh], taps)             # [B, ncol, L]
    hi, lo = planes.start_fold_sets(win, False, nwc, 1)                 # [B, 32 * nwc, L]
    wh, wl = torch.zeros_like(Wh), torch.zeros_like(Wl)
    wh[:, :, halo:halo + L] = hi.view(B, nwc, 32, L).permute(0, 1, 3, 2)
    wl[:, :, halo:halo + L] = lo.view(B, nwc, 32, L).permute(0, 1, 3, 2)
    assert torch.equal(Wh, wh) and torch.equal(Wl, wl)
    # spelled out for set 0: the ones-channel is 1 at the centre tap everywhere, 0 where an edge tap leaves the utterance
    v = (Wh[:, 0, halo:halo + L, :ncol].float() + Wl[:, 0, halo:halo + L, :ncol].float()).permute(0, 2, 1)
    assert bool((v[:, (taps // 2) * (nh + 1) + nh] == 1.0).all())
    assert bool((v[:, nh, :taps // 2] == 0.0).all()) and bool((v[:, (taps - 1) * (nh + 1) + nh, L - (taps // 2):] == 0.0).all())
    # the four sets add up to the f32 window value
    tot = (hi.double() + lo.double()).view(B, nwc * 32, L)
    rec = sum(tot[:, _set_cols(s_, ncol, nwc):_set_cols(s_, ncol, nwc) + ncol] for s_ in (0, 2))
    assert float((rec.cpu() - win.double().cpu()).abs().max()) <= 2.0 ** -30 * float(win.abs().max())


@pytest.mark.parametrize("cfg_name,flows", [("small", (0, 5, 11)), ("default", (0, 4, 8))])
def test_composed_block_vs_f64(cfg_name, flows):
    """(b) The composed weight in the layer-0 operand against (g / |v|) v_in0[:, :, tap] . [w_start | b_start] computed in f64 and put
    through the same row permutation.  Column set 0 - the plain split-bf16 pair - at the bars test_waveglow_gpu.py::test_wn_layer
    puts on split-bf16 results (rel-L2 2e-5, max 1e-4 of the largest value); sets 0 + 1 (the pair plus its residual) are printed
    and must not be worse; sets 2 and 3 are bit-for-bit (h, l) and (l, 0) of set 0; rows past 2C and unused columns are zero.  The
    chunks behind them and the bias are bit-for-bit what the unfolded pack writes for the conditioning layer."""
    from oracle import waveglow_oracle as O
    cfg = synth.WAVEGLOW_SMALL if cfg_name == "small" else synth.WAVEGLOW_DEFAULT
    sd = synth.waveglow_state(cfg)
    m = _build(cfg, sd)
    eng = m._eng()
    g = eng.geom()
    C, ks, nwc = g["C"], g["ks"], g["nwc"]
    eng.pack_weights(torch.device(DEV), force=True, res_pair8=True, start_fold=False)
    torch.cuda.synchronize()
    plain = {k: (eng.packed["flows"][k]["layers"][0]["A1h"][ks * g["Cpad"] // 32:].clone(),
                 eng.packed["flows"][k]["layers"][0]["A1l"][ks * g["Cpad"] // 32:].clone(),
                 eng.packed["flows"][k]["layers"][0]["b1"].clone()) for k in flows}
    eng.pack_weights(torch.device(DEV), force=True, res_pair8=True, start_fold=True)
    torch.cuda.synchronize()
    assert eng.packed["start_fold"]
    sd64 = {n: t.double() for n, t in sd.items()}
    rows = torch.tensor([_gate_row(o, C) for o in range(2 * C)])
    for k in flows:
        fl = eng.packed["flows"][k]
        nh = fl["n_half"]
        ncol = ks * (nh + 1)
        p = "WN.%d." % k
        M = planes.start_fold_matrix(O.effective_weight(sd64, p + "in_layers.0"), O.effective_weight(sd64, p + "start"),
                                     sd64[p + "start.bias"])
        want = torch.zeros(g["Mpad1"], ncol, dtype=torch.float64)
        want[rows] = M
        Ah = fl["A0h"][:nwc].permute(1, 0, 2).reshape(g["Mpad1"], nwc * 32).cpu()
        Al = fl["A0l"][:nwc].permute(1, 0, 2).reshape(g["Mpad1"], nwc * 32).cpu()
        sets = [(Ah[:, _set_cols(s_, ncol, nwc):_set_cols(s_, ncol, nwc) + ncol], Al[:, _set_cols(s_, ncol, nwc):_set_cols(s_, ncol, nwc) + ncol])
                for s_ in range(4)]
        got = sets[0][0].double() + sets[0][1].double()
        fine = got + sets[1][0].double() + sets[1][1].double()
        r, mx, rf = _rel(got, want), _maxrel(got, want), _rel(fine, want)
        print("%s flow %d (n_half %d): composed block rel %.2e max %.2e; with its residual set rel %.2e" % (cfg_name, k, nh, r, mx, rf))
        assert r < 2e-5 and mx < 1e-4, (k, r, mx)
        assert rf <= r
        assert torch.equal(sets[2][0], sets[0][0]) and torch.equal(sets[2][1], sets[0][1])
        assert torch.equal(sets[3][0], sets[0][1]) and float(sets[3][1].float().abs().max()) == 0.0
        used = torch.zeros(nwc * 32, dtype=torch.bool)
        for s_ in range(4):
            used[_set_cols(s_, ncol, nwc):_set_cols(s_, ncol, nwc) + ncol] = True
        assert float(Ah[:, ~used].float().abs().max()) == 0.0 and float(Al[:, ~used].float().abs().max()) == 0.0
        unused = torch.ones(g["Mpad1"], dtype=torch.bool)
        unused[rows] = False
        if bool(unused.any()):
            assert float(Ah[unused].float().abs().max()) == 0.0
        assert torch.equal(fl["A0h"][nwc:], plain[k][0]) and torch.equal(fl["A0l"][nwc:], plain[k][1])
        assert torch.equal(fl["layers"][0]["b1"], plain[k][2])


def _both(monkeypatch, fn):
    """fn() with the fold on, then with T2S_START_FOLD=0; checks that each run took the path it was asked for"""
    out = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("T2S_START_FOLD", flag)
        out[flag] = fn(flag == "1")
    monkeypatch.delenv("T2S_START_FOLD")
    return out["1"], out["0"]


def test_wn_forward_fold_on_vs_off_vs_oracle(monkeypatch):
    """(c) WN[k].forward for flows with n_half = 4, 3, 2: fold on against the oracle at test_submodules_gpu.py's bar (rel 1e-3), and
    against T2S_START_FOLD=0 at the bar test_edge_cases_gpu.py puts on two kernel paths over the same inputs (rel 2e-5).
    Measured on MI355X (profiles/start_fold_tests.txt): fold on versus off rel 4.4e-6 / 4.4e-6 / 4.5e-6 for flows 0 / 5 / 11; against
    the oracle 8.2e-6 / 8.2e-6 / 8.4e-6 with the fold and 8.3e-6 / 8.4e-6 / 8.6e-6 without.  forward() at the small config: z on
    versus off 1.9e-6, worst log_s 4.9e-6; infer() audio 1.5e-6 to 2.5e-6; 128-row tiles: z 2.0e-6, audio 1.6e-6."""
    from oracle import waveglow_oracle as O
    cfg = synth.WAVEGLOW_SMALL
    sd = synth.waveglow_state(cfg)
    m = _build(cfg, sd)
    eng = m._eng()
    gen = torch.Generator().manual_seed(3)
    B, L = 2, 600
    for k in (0, 5, 11):
        n_half = m.WN[k].start.in_channels
        audio = torch.randn(B, n_half, L, generator=gen)
        spect = torch.randn(B, 640, L, generator=gen)

        def run(on):
            got = m.WN[k]((audio.to(DEV), spect.to(DEV)))
            assert bool(eng.packed["start_fold"]) == on
            return got
        on, off = _both(monkeypatch, run)
        with torch.no_grad():
            want = O.wn_forward(sd, cfg, k, audio, spect)
        d, ron, roff = _rel(on, off), _rel(on, want), _rel(off, want)
        print("WN[%d] (n_half %d): fold on vs off rel %.2e; vs oracle on %.2e off %.2e" % (k, n_half, d, ron, roff))
        assert ron < 1e-3, (k, ron)
        assert d < 2e-5, (k, d)


@pytest.mark.parametrize("name,batch,n,seed", [
    ("waveglow_small_fwd", 2, 4096, 31),
    ("waveglow_small_ragged_fwd", 3, 2400, 32),
])
def test_forward_small_fold_on_vs_off_golden_oracle(monkeypatch, golden_dir, name, batch, n, seed):
    """(c) forward() at the small config: the bars of test_waveglow_gpu.py::test_forward_small_vs_golden with the fold on, and
    fold on against T2S_START_FOLD=0 at 2e-5 (the bar between two kernel paths, test_edge_cases_gpu.py)."""
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
        assert bool(eng.packed["start_fold"]) == on
        return out
    (z, log_s, log_det), (z0, log_s0, _) = _both(monkeypatch, run)
    with torch.no_grad():
        zo, lso, ldo = O.waveglow_forward(synth.waveglow_state(cfg), cfg, mel, audio)
    d = _rel(z, z0)
    dls = max(_rel(a, b) for a, b in zip(log_s, log_s0))
    print("%s: fold on vs off z rel %.2e, worst log_s rel %.2e; z vs golden on %.2e off %.2e" % (name, d, dls, _rel(z, g["z"]), _rel(z0, g["z"])))
    assert _rel(z, g["z"]) < 1e-3 and _maxrel(z, g["z"]) < 1e-3
    assert _rel(z, g["z"]) < 1e-4
    assert _rel(z, zo) < 1e-4
    np.testing.assert_allclose([float(x) for x in log_det], g["log_det"], rtol=1e-4, atol=1e-2)
    for k, ls in enumerate(log_s):
        assert _rel(ls, lso[k]) < 1e-3, "flow %d log_s" % k
    assert d < 2e-5 and dls < 2e-5, (d, dls)


@pytest.mark.parametrize("name,sigma", [("waveglow_small_infer_s0", 0.0), ("waveglow_small_infer_s0666", 0.666)])
def test_infer_small_fold_on_vs_off_golden(monkeypatch, golden_dir, name, sigma):
    """(c) infer() at the small config: test_waveglow_gpu.py::test_infer_small_vs_golden's bar with the fold on, and on-vs-off at 2e-5."""
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    cfg = synth.WAVEGLOW_SMALL
    m = _build(cfg)
    eng = m._eng()
    gen = torch.Generator().manual_seed(41)
    mel = torch.randn(2, 80, 12, generator=gen)
    noise = (torch.from_numpy(g["noise_final"]), [torch.from_numpy(g[f"noise_early_{i}"]) for i in range(2)])

    def run(on):
        a = m.infer(mel.to(DEV), sigma=sigma, noise=noise)
        assert bool(eng.packed["start_fold"]) == on
        return a
    a_on, a_off = _both(monkeypatch, run)
    d = _rel(a_on, a_off)
    print("%s: fold on vs off audio rel %.2e; vs golden on %.2e off %.2e" % (name, d, _rel(a_on, g["audio"]), _rel(a_off, g["audio"])))
    assert tuple(a_on.shape) == g["audio"].shape
    assert _rel(a_on, g["audio"]) < 1e-3 and _maxrel(a_on, g["audio"]) < 1e-3
    assert d < 2e-5, d


def test_stress_weights_fold_on_vs_off_vs_oracle(monkeypatch):
    """(c) the stress weights of test_waveglow_gpu.py::test_stress_weights_forward_and_infer_vs_oracle (WN.end std 0.03, every
    weight-norm gain x 1.25, config.json defaults, 2 x 4096 samples and a 24-frame infer) with the fold on, at that test's bar:
    z, every log_s and the audio within 1e-3 (rel-L2 and max) of the f32 oracle.  The fold-on versus fold-off difference is
    printed next to both paths' errors (it is a difference between two roundings of an ill-conditioned flow, so it is bounded by the
    same 1e-3 and not by the 2e-5 of the seeded weights).
    Measured on MI355X (profiles/start_fold_tests.txt), fold on (fold off): infer audio rel 3.4e-4 (3.2e-4), max 5.2e-4 (6.5e-4) -
    a margin of 1.9x to the 1e-3 bar; z rel 1.4e-4 (1.4e-4), max 2.2e-4 (3.3e-4); worst log_s 1.5e-4 (1.4e-4); on versus off
    z 8.2e-5, log_s 9.9e-5, audio 4.1e-4.  A first form of the fold with one plain split-bf16 column set put the audio maximum at
    1.01e-3, over the bar (profiles/start_fold_v1_single_set.txt); the four column sets are the answer to that."""
    from oracle import waveglow_oracle as O
    cfg = synth.WAVEGLOW_DEFAULT
    sd = synth.waveglow_state(cfg, end_std=0.03, wn_gain=1.25)
    m = _build(cfg, sd)
    eng = m._eng()
    mel, audio = synth.waveglow_inputs(2, 4096, seed=31)
    gen = torch.Generator().manual_seed(5)
    frames = 24
    mel_inf = torch.randn(1, 80, frames, generator=gen)
    L = frames * 256 // 8
    noise = (torch.randn(1, 4, L, generator=gen), [torch.randn(1, 2, L, generator=gen) for _ in range(2)])

    def run(on):
        with torch.no_grad():
            z, log_s, _ = m((mel.to(DEV), audio.to(DEV)))
            assert bool(eng.packed["start_fold"]) == on
            a = m.infer(mel_inf.to(DEV), sigma=0.666, noise=noise)
            assert bool(eng.packed["start_fold"]) == on
        torch.cuda.synchronize()
        return z, log_s, a
    (z, log_s, a), (z0, log_s0, a0) = _both(monkeypatch, run)
    with torch.no_grad():
        zo, lso, _ = O.waveglow_forward(sd, cfg, mel, audio)
        ao = O.waveglow_infer(sd, cfg, mel_inf, noise[0], noise[1], sigma=0.666)
    assert max(float(l.abs().max()) for l in lso) > 2.5          # the stress is real
    rz, mz = _rel(z, zo), _maxrel(z, zo)
    worst_ls = max(_rel(x, y) for x, y in zip(log_s, lso))
    ra, ma = _rel(a, ao), _maxrel(a, ao)
    print("stress weights, fold on : z rel %.1e max %.1e, worst log_s rel %.1e, infer audio rel %.1e max %.1e" % (rz, mz, worst_ls, ra, ma))
    print("stress weights, fold off: z rel %.1e max %.1e, worst log_s rel %.1e, infer audio rel %.1e max %.1e"
          % (_rel(z0, zo), _maxrel(z0, zo), max(_rel(x, y) for x, y in zip(log_s0, lso)), _rel(a0, ao), _maxrel(a0, ao)))
    print("stress weights, on vs off: z rel %.1e, worst log_s rel %.1e, audio rel %.1e"
          % (_rel(z, z0), max(_rel(x, y) for x, y in zip(log_s, log_s0)), _rel(a, a0)))
    assert rz < 1e-3 and mz < 1e-3, (rz, mz)
    assert worst_ls < 1e-3, worst_ls
    assert ra < 1e-3 and ma < 1e-3, (ra, ma)
    assert _rel(z, z0) < 1e-3 and _rel(a, a0) < 1e-3


def test_short_utterance_takes_128_row_tiles(monkeypatch):
    """(d) B = 1, 139 frames at the small config: the folded gate GEMM - layer 0 with its 22 K-steps included - runs on the 128-row
    lockstep tiles (test_edge_cases_gpu.py::test_waveglow_gate_tile_heights's short case and bars), forward and inverse."""
    from oracle import waveglow_oracle as O
    lib = _lib.load()
    cfg = synth.WAVEGLOW_SMALL
    B, frames = 1, 139
    T = 256 * (frames - 1)
    L = T // cfg["n_group"]
    assert lib.t2s_wg_gate_tile_rows(B, cfg["WN_config"]["n_channels"], L) == 128
    m = _build(cfg)
    eng = m._eng()
    gen = torch.Generator().manual_seed(frames + B)
    mel = torch.randn(B, 80, frames, generator=gen)
    audio = torch.rand(B, T, generator=gen) - 0.5
    fr = 40
    Li = 256 * fr // cfg["n_group"]
    assert lib.t2s_wg_gate_tile_rows(B, cfg["WN_config"]["n_channels"], Li) == 128
    nf = torch.randn(B, 4, Li, generator=gen)
    ne = [torch.randn(B, 2, Li, generator=gen) for _ in range(2)]

    def run(on):
        with torch.no_grad():
            z, log_s, _ = m((mel.to(DEV), audio.to(DEV)))
            assert bool(eng.packed["start_fold"]) == on
            a = m.infer(mel[:, :, :fr].to(DEV), sigma=0.5, noise=(nf, ne))
        return z, log_s, a
    (z, log_s, a), (z0, _, a0) = _both(monkeypatch, run)
    with torch.no_grad():
        zo, lso, _ = O.waveglow_forward(synth.waveglow_state(cfg), cfg, mel, audio)
        ao = O.waveglow_infer(synth.waveglow_state(cfg), cfg, mel[:, :, :fr], nf, ne, sigma=0.5)
    print("128-row tiles: z vs oracle %.2e, audio vs oracle %.2e; fold on vs off z %.2e audio %.2e"
          % (_rel(z, zo), _rel(a, ao), _rel(z, z0), _rel(a, a0)))
    assert _rel(z, zo) < 1e-4
    for x, y in zip(log_s, lso):
        assert _rel(x, y) < 1e-3
    assert _rel(a, ao) < 1e-3
    assert _rel(z, z0) < 2e-5 and _rel(a, a0) < 2e-5


def test_fallback_when_the_taps_do_not_fit(monkeypatch):
    """(e) kernel_size 7: 7 * (4 + 1) = 35 window columns do not fit a 32-wide K-step, so the engine keeps the unfolded layer 0
    (packed["start_fold"] is False) - forward against the oracle at the small-config bars.  kernel_size 5 (25 columns) folds with four window chunks
    at 128 channels, and falls back at 64 (two channel chunks only)."""
    from oracle import waveglow_oracle as O
    monkeypatch.delenv("T2S_START_FOLD", raising=False)
    for ks, C, folds in ((7, 64, False), (5, 128, True), (5, 64, False)):
        cfg = dict(synth.WAVEGLOW_SMALL, n_flows=4, WN_config=dict(n_layers=4, n_channels=C, kernel_size=ks))
        sd = synth.waveglow_state(cfg)
        m = _build(cfg, sd)
        eng = m._eng()
        assert eng.start_fold_on() == folds
        mel, audio = synth.waveglow_inputs(2, 4096, seed=33)
        with torch.no_grad():
            z, log_s, _ = m((mel.to(DEV), audio.to(DEV)))
            zo, lso, _ = O.waveglow_forward(sd, cfg, mel, audio)
        torch.cuda.synchronize()
        assert bool(eng.packed["start_fold"]) == folds
        print("kernel_size %d, %d channels (fold %s): z vs oracle %.2e" % (ks, C, folds, _rel(z, zo)))
        assert _rel(z, zo) < 1e-4
        for x, y in zip(log_s, lso):
            assert _rel(x, y) < 1e-3
