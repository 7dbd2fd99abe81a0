"""What each no-grad kernel path launches, counted at the C ABI: _lib.call is wrapped so that it records the
entry point's name and then calls through - the kernels run, the outputs are checked for finiteness - and the counts per call of
forward() and infer() are compared with the table below.  "Which path ran" then rests on the launches, not on a flag the engine
sets for itself; eng.last_path is checked against the same table.

F flows, N layers; counts are forward / infer:

    entry point                  A: default           B: T2S_FLOW_BOUNDARY=0   C: T2S_START_FOLD=0 (and D: kernel_size 7)
    t2s_wg_flow_boundary         F / F                0 / 0                    0 / 0
    t2s_wg_start_window          0 / 0                F / F                    0 / 0
    t2s_wg_start                 0 / 0                0 / 0                    F / F
    t2s_wg_convinv               0 / F                F / F                    F / F
    t2s_wg_in_win_gate_fold      F / F                F / F                    0 / 0
    t2s_wg_in_cond_gate_fold     F(N-1) / F(N-1)      F(N-1) / F(N-1)          FN / FN
    t2s_wg_res_only_start        F / F                0 / 0                    0 / 0
    t2s_wg_res_only              F(N-2) / F(N-2)      F(N-1) / F(N-1)          F(N-1) / F(N-1)
    t2s_wg_end_fold_affine       1 / F                F / F                    F / F

The two fp16 chains of a .half() model (infer with infer_w16 = True, infer_batch with infer_batch_w16 = True; path
(False, False, None)) launch, per call:

    E: infer                              F: infer_batch                                  count
    t2s_wg_upsample_squeeze_h16           t2s_wg_upsample_squeeze_h16                     1
    t2s_wg_start_h16                      t2s_wg_start_h16_ragged                         F
    t2s_wg_in_cond_gate_fold_h16          t2s_wg_in_cond_gate_fold_h16_ragged             FN
    t2s_wg_res_only_h16                   t2s_wg_res_only_h16_ragged                      F(N-1)
    t2s_wg_end_fold_affine, t2s_wg_convinv                                                F each
    t2s_wg_audio_squeeze                  ... and t2s_zero_rows_f32                       1 each

and the first call of a model also t2s_pack_conv_weight_table_h16, t2s_wg_endfold_weights_h16, t2s_weightnorm_small and
t2s_small_logdet_inv, F each; none of the split-bf16 entry points of the table above.
"""
import collections

import pytest
import torch

from text2speech_amd import _lib, synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# the kernel-size-7 configuration of tests/test_start_fold_gpu.py::test_fallback_when_the_taps_do_not_fit: 35 window columns
CFG_KS7 = dict(synth.WAVEGLOW_SMALL, n_flows=4, WN_config=dict(n_layers=4, n_channels=64, kernel_size=7))
# no no-grad call reaches the unfolded gate / res-skip GEMMs or the unfolded WN.end
NEVER = ("t2s_wg_in_cond_gate", "t2s_wg_res_skip", "t2s_wg_end_affine")


def _want(case, F, N):
    """(forward counts, infer counts, last_path) of the table in the module docstring"""
    if case == "A":
        fwd = dict(t2s_wg_flow_boundary=F, t2s_wg_start_window=0, t2s_wg_start=0, t2s_wg_convinv=0, t2s_wg_in_win_gate_fold=F,
                   t2s_wg_in_cond_gate_fold=F * (N - 1), t2s_wg_res_only_start=F, t2s_wg_res_only=F * (N - 2), t2s_wg_end_fold_affine=1)
        return fwd, dict(fwd, t2s_wg_convinv=F, t2s_wg_end_fold_affine=F), (True, True, None)
    if case == "B":
        both = dict(t2s_wg_flow_boundary=0, t2s_wg_start_window=F, t2s_wg_start=0, t2s_wg_convinv=F, t2s_wg_in_win_gate_fold=F,
                    t2s_wg_in_cond_gate_fold=F * (N - 1), t2s_wg_res_only_start=0, t2s_wg_res_only=F * (N - 1), t2s_wg_end_fold_affine=F)
        return both, both, (True, False, None)
    both = dict(t2s_wg_flow_boundary=0, t2s_wg_start_window=0, t2s_wg_start=F, t2s_wg_convinv=F, t2s_wg_in_win_gate_fold=0,
                t2s_wg_in_cond_gate_fold=F * N, t2s_wg_res_only_start=0, t2s_wg_res_only=F * (N - 1), t2s_wg_end_fold_affine=F)
    return both, both, (False, False, None)


@pytest.mark.parametrize("case,cfg,env", [
    ("A", synth.WAVEGLOW_SMALL, {}),
    ("B", synth.WAVEGLOW_SMALL, {"T2S_FLOW_BOUNDARY": "0"}),
    ("C", synth.WAVEGLOW_SMALL, {"T2S_START_FOLD": "0"}),
    ("D", CFG_KS7, {}),
])
def test_launches_per_path(monkeypatch, case, cfg, env):
    """B = 1, 2048 samples (L = 256) through forward() and 8 mel frames through infer(): the smallest grids every kernel accepts,
    the subject being the host's sequence.  One forward with eng.gemm_events = [] and stride 1 appends one event pair per full-K gate
    launch: F(N-1) where layer 0 is folded (A, B), FN where it is not (C, D)."""
    from text2speech_amd.glow import WaveGlow
    for name in ("T2S_START_FOLD", "T2S_FLOW_BOUNDARY", "T2S_COND_COMPOSE"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    m = WaveGlow(**cfg)
    m.load_state_dict(synth.waveglow_state(cfg), strict=True)
    m = m.to(DEV).eval()
    eng = m._eng()
    F, N = m.n_flows, m.WN[0].n_layers
    want_fwd, want_inf, want_path = _want(case, F, N)

    seen = collections.Counter()
    real_call = _lib.call

    def counting_call(name, *args):
        seen[name] += 1
        return real_call(name, *args)
    monkeypatch.setattr(_lib, "call", counting_call)

    mel, audio = synth.waveglow_inputs(1, 2048, seed=61)
    eng.gemm_events, eng.gemm_event_stride = [], 1
    with torch.no_grad():
        z, log_s, _ = m((mel.to(DEV), audio.to(DEV)))
    torch.cuda.synchronize()
    n_pairs, eng.gemm_events = len(eng.gemm_events), None
    got_fwd = {name: seen[name] for name in want_fwd}
    print("case %s forward (F %d, N %d): %r, %d event pairs, path %r" % (case, F, N, got_fwd, n_pairs, eng.last_path))
    assert eng.last_path == want_path
    assert got_fwd == want_fwd
    assert not any(seen[name] for name in NEVER), seen
    assert n_pairs == (F * (N - 1) if case in "AB" else F * N)
    assert bool(torch.isfinite(z).all()) and all(bool(torch.isfinite(t).all()) for t in log_s)

    seen.clear()
    a = m.infer(mel[:, :, :8].to(DEV), sigma=0.6)
    torch.cuda.synchronize()
    got_inf = {name: seen[name] for name in want_inf}
    print("case %s infer: %r, path %r" % (case, got_inf, eng.last_path))
    assert eng.last_path == want_path
    assert got_inf == want_inf
    assert not any(seen[name] for name in NEVER), seen
    assert tuple(a.shape) == (1, 2048) and bool(torch.isfinite(a).all())


# what only a call on split-bf16 planes launches, and the four entry points of infer_batch on them
BF16 = ("t2s_wg_upsample_squeeze", "t2s_wg_start", "t2s_wg_start_window", "t2s_wg_flow_boundary", "t2s_wg_in_win_gate_fold",
        "t2s_wg_in_cond_gate_fold", "t2s_wg_res_only", "t2s_wg_res_only_start", "t2s_wg_startfold_weights",
        "t2s_pack_conv_weight_table", "t2s_wg_endfold_weights")
BF16_RAGGED = ("t2s_wg_start_ragged", "t2s_wg_res_only_ragged", "t2s_wg_res_only_start_ragged", "t2s_wg_flow_boundary_ragged")
H16_CHAIN = ("t2s_wg_start_h16", "t2s_wg_in_cond_gate_fold_h16", "t2s_wg_res_only_h16")
H16_PACK = ("t2s_pack_conv_weight_table_h16", "t2s_wg_endfold_weights_h16", "t2s_weightnorm_small", "t2s_small_logdet_inv")


@pytest.mark.parametrize("case", ["E", "F"])
def test_launches_of_the_fp16_chains(monkeypatch, case):
    """The small model as .half() with the 1x1 convolutions put back to float, twice through infer (E: B = 1, 8 frames) or
    infer_batch (F: 8 and 3 frames, L = 256 columns, entries of 256 and 96) with the switch set to True and the same seeded noise:
    the launches of the second table in the module docstring, the pack on the first call only, the same bits on the second."""
    from text2speech_amd.glow import WaveGlow
    for name in ("T2S_START_FOLD", "T2S_FLOW_BOUNDARY", "T2S_COND_COMPOSE"):
        monkeypatch.delenv(name, raising=False)
    cfg = synth.WAVEGLOW_SMALL
    m = WaveGlow(**cfg)
    m.load_state_dict(synth.waveglow_state(cfg), strict=True)
    m = m.to(DEV).eval().half()
    for c in m.convinv:
        c.float()
    eng = m._eng()
    F, N = m.n_flows, m.WN[0].n_layers
    B = 1 if case == "E" else 2
    rag = "" if case == "E" else "_ragged"
    want = {"t2s_wg_upsample_squeeze_h16": 1, "t2s_wg_end_fold_affine": F, "t2s_wg_convinv": F, "t2s_wg_audio_squeeze": 1,
            "t2s_zero_rows_f32": 1 if case == "F" else 0, "t2s_zero_plane_rows": 0}
    want.update(zip((n + rag for n in H16_CHAIN), (F, F * N, F * (N - 1))))
    if case == "F":
        want.update(dict.fromkeys(H16_CHAIN, 0))

    seen = collections.Counter()
    real_call = _lib.call

    def counting_call(name, *args):
        seen[name] += 1
        return real_call(name, *args)
    monkeypatch.setattr(_lib, "call", counting_call)

    mel = synth.waveglow_inputs(B, 2048, seed=67)[0][:, :, :8].to(DEV)
    gen = torch.Generator().manual_seed(68)
    noise = (torch.randn(B, 4, 256, generator=gen).to(DEV), [torch.randn(B, 2, 256, generator=gen).to(DEV) for _ in range(2)])
    audio = []
    for first in (True, False):
        seen.clear()
        try:
            if case == "E":
                eng.infer_w16 = True
                a = m.infer(mel, sigma=0.6, noise=noise)
            else:
                eng.infer_batch_w16 = True
                a, _ = m.infer_batch(mel, [8, 3], sigma=0.6, noise=noise)
        finally:
            eng.infer_w16, eng.infer_batch_w16 = None, False
        torch.cuda.synchronize()
        audio.append(a)
        got = {name: seen[name] for name in want}
        print("case %s call %d: %r, pack %r, path %r" % (case, 2 - first, got, {n: seen[n] for n in H16_PACK}, eng.last_path))
        assert eng.last_path == (False, False, None)
        assert eng.last_infer_w16 is True and eng.last_infer_batch_w16 is (case == "F")
        assert got == want
        assert {n: seen[n] for n in H16_PACK} == dict.fromkeys(H16_PACK, F if first else 0)
        assert not any(seen[name] for name in BF16 + BF16_RAGGED + NEVER), seen
        if case == "E":
            assert not any(name.endswith("_ragged") for name in seen), seen
        assert tuple(a.shape) == (B, 2048) and a.dtype == torch.float32 and bool(torch.isfinite(a).all())
    assert torch.equal(audio[0], audio[1])
    if case == "F":
        assert not bool(audio[0][1, 3 * 256:].any()) and bool(audio[0][1, :3 * 256].any())
