"""CPU-side checks of the C-ABI boundary: the library builds/loads without a GPU and exports every
symbol that include/t2s_hip.h declares; the ctypes table covers them all.  No compute calls."""
import os
import re

import pytest

from text2speech_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def _declared():
    src = open(os.path.join(ROOT, "include", "t2s_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(t2s_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_exported(lib):
    names = _declared()
    assert len(names) >= 15
    for n in names:
        assert hasattr(lib, n), "libt2s_hip.so does not export %s" % n


def test_ctypes_table_matches_header():
    assert sorted(_lib.SIGNATURES) == _declared()


def test_pure_host_entry_points(lib):
    assert lib.t2s_abi_version() == 4      # round 4: t2s_taco_decoder grew (gate_part, w_pre2T); INTEGRATION.md lists what changed per version
    import ctypes
    from text2speech_amd.tacotron.tacotron import _DecoderStruct
    assert lib.t2s_sizeof_taco_decoder() == ctypes.sizeof(_DecoderStruct)       # the ctypes mirrors against the compiled structs
    from text2speech_amd.tacotron.autograd import _Bptt
    assert lib.t2s_sizeof_taco_bptt() == ctypes.sizeof(_Bptt)
    assert lib.t2s_plane_rows(2000, 128) == 2048 + 256
    assert lib.t2s_plane_rows(256, 0) == 256
    assert lib.t2s_padded_rows(1024) == 1024 and lib.t2s_padded_rows(130) == 256
    assert lib.t2s_error_string(0) == b"ok"
    assert lib.t2s_error_string(-1) == b"invalid argument"
    # gate-GEMM tile height by grid size: 256-row tiles above 128 workgroups, 128-row tiles (twice the fold slots) below
    assert lib.t2s_wg_gate_fold_slots(8, 512, 2000) == 8          # 4 x 8 x 8 = 256 workgroups of 256-row tiles
    assert lib.t2s_wg_gate_fold_slots(1, 512, 6400) == 16         # 4 x 25 = 100 workgroups -> 128-row tiles
    assert lib.t2s_wg_gate_fold_slots(1, 512, 32000) == 8
    assert lib.t2s_wg_gate_fold_slots(0, 512, 10) == -1


def test_argument_validation_without_gpu(lib):
    # null pointers / bad geometry are rejected before anything touches the device
    assert lib.t2s_wg_convinv(None, None, 1, 8, 0, 8, 10, None) == -1
    assert lib.t2s_small_logdet_inv(None, 4, 1.0, None, None, None) == -1
    assert lib.t2s_pack_conv_weight(None, None, 0, None, 4, 4, 1, 0, 0, 0, 256, 0, 32, None, None, None, 0, None) == -1
    assert lib.t2s_wg_melwin_planes(None, 1, 80, 10, 4, 256, None, None, None) == -1
    assert lib.t2s_wg_upsample_basis(None, None, 80, 1024, 256, 8, 0, 0, None, None, None) == -1
    assert lib.t2s_wg_compose_cond(None, None, 1024, 1024, 32, 320, 10241, None, None, None, None) == -1


def test_composed_conditioning_is_opt_in(monkeypatch):
    """Host logic of the inverse flow's composed-conditioning path: off unless T2S_COND_COMPOSE=1, and
    only for geometries where the upsampler's hop is a whole number of plane rows and the mel window fills whole 32-channel chunks."""
    from text2speech_amd import synth
    from text2speech_amd.glow import WaveGlow
    m = WaveGlow(**synth.WAVEGLOW_SMALL)
    eng = m._eng()
    monkeypatch.delenv("T2S_COND_COMPOSE", raising=False)
    assert eng.compose_geom() is None
    monkeypatch.setenv("T2S_COND_COMPOSE", "1")
    assert eng.compose_geom() == (32, 4, 320)          # hop 256 / n_group 8 phases, 1024 / 256 lags, 4 x 80 window channels
    monkeypatch.setenv("T2S_COND_COMPOSE", "0")
    assert eng.compose_geom() is None


# The sixteen conv-GEMM entry points, parameters in ABI order (the c_void_p slots of _lib.SIGNATURES are the pointers).
_GEMM_ENTRIES = {
    "t2s_wg_in_cond_gate": "A_hi A_lo bias X_hi X_lo S_hi S_lo acts_hi acts_lo B C n_cond taps dilation L Lp halo Mpad stream",
    "t2s_wg_res_skip": "A_hi A_lo bias acts_hi acts_lo X_hi X_lo skip B C n_res skip_init L Lp halo Mpad stream",
    "t2s_wg_in_cond_gate_fold": "A_hi A_lo bias X_hi X_lo S_hi S_lo acts_hi acts_lo fold_A fold_acc fold_init B C n_cond taps dilation "
                                "L Lp halo Mpad stream",
    "t2s_wg_in_win_gate_fold": "A_hi A_lo bias W_hi W_lo S_hi S_lo acts_hi acts_lo fold_A fold_acc fold_init B C n_cond win_chunks "
                               "L Lp halo Mpad stream",
    "t2s_wg_in_melwin_gate_fold": "A_hi A_lo A2_hi A2_lo bias X_hi X_lo M_hi M_lo acts_hi acts_lo fold_A fold_acc fold_init B C K2 "
                                  "taps dilation L Lp halo Mpad P Fp stream",
    "t2s_wg_res_only": "A_hi A_lo bias acts_hi acts_lo X_hi X_lo B C L Lp halo Mpad pair8 stream",
    "t2s_conv_bias_act": "A_hi A_lo bias X_hi X_lo O_hi O_lo out_f32 f32_channel_last B Cin C taps dilation act L Lp halo Mpad stream",
    "t2s_wg_in_cond_gate_train": "A_hi A_lo bias X_hi X_lo S_hi S_lo acts_hi acts_lo T_hi T_lo G_hi G_lo B C n_cond taps dilation "
                                 "L Lp halo Mpad stream",
    "t2s_wg_in_cond_gate_fold_train": "A_hi A_lo bias X_hi X_lo S_hi S_lo acts_hi acts_lo G_hi G_lo act_bchunks fold_A fold_acc "
                                      "fold_init B C n_cond taps dilation L Lp halo Mpad stream",
    "t2s_wg_res_only_train": "A_hi A_lo bias acts_hi acts_lo act_bchunks R_hi R_lo X_hi X_lo B C L Lp halo Mpad pair8 stream",
    "t2s_wg_skip_sum": "A_hi A_lo bias acts_hi acts_lo n_k_chunks act_bchunks skip B C L Lp halo Mpad stream",
    "t2s_wg_res_skip_train": "A_hi A_lo bias acts_hi acts_lo R_hi R_lo X_hi X_lo skip B C n_res skip_init L Lp halo Mpad stream",
    "t2s_wg_bwd_gate_dgrad": "A_hi A_lo zero_bias DX_hi DX_lo DS_hi DS_lo T_hi T_lo G_hi G_lo tg_bchunks DP_hi DP_lo dp_bchunks B C "
                             "L Lp halo Mpad pair8 stream",
    "t2s_conv_accumulate": "A_hi A_lo zero_bias X_hi X_lo x_bchunks O_hi O_lo B Cin C taps dilation init L Lp halo Mpad pair8 stream",
    "t2s_wgrad_gemm": "A_hi A_lo X_hi X_lo zero_bias out B C L Mpad Lp n_tchunks k0 k1 ksplit stream",
    "t2s_wgrad_gemm_flat": "A_hi A_lo X_hi X_lo zero_bias out B C L Mpad Lp n_tchunks k0 k1 nsplit stream",
}
# "C" is the entry's output-row count (C, Cout or M) and "L" its column count (L or N).  A valid small shape: two batch entries,
# two 32-channel chunks, two column tiles; integers not named here (the flags and the *_bchunks strides) are 0.
_GEMM_BASE = dict(B=2, C=64, Cin=64, n_cond=80, n_res=64, taps=3, dilation=2, L=300, halo=4, Lp=520, Mpad=256, win_chunks=2, K2=64,
                  P=4, Fp=80, n_tchunks=3, k0=0, k1=3, ksplit=2, nsplit=2, n_k_chunks=2)
# the phase-mode gate refuses shapes whose tile height is 128 (C = 64 here); the weight-gradient planes have no halo
_GEMM_BASE_OF = {"t2s_wg_in_melwin_gate_fold": dict(C=80),
                 "t2s_wgrad_gemm": dict(Lp=512), "t2s_wgrad_gemm_flat": dict(Lp=512)}
_NULL_ALLOWED = {"out_f32", "DX_hi", "stream"}                            # optional outputs / operands
_UNALIGNED_ALLOWED = {"fold_acc", "zero_bias", "out", "out_f32", "stream"}


def _gemm_args(name, **changes):
    """Argument tuple of a conv-GEMM entry point: made-up, distinct, 16-byte-aligned pointers and the base shape, then `changes`."""
    import ctypes
    vals = dict(_GEMM_BASE, **_GEMM_BASE_OF.get(name, {}))
    vals.update(changes)
    params = _GEMM_ENTRIES[name].split()
    assert len(params) == len(_lib.SIGNATURES[name])
    out = []
    for i, (p, t) in enumerate(zip(params, _lib.SIGNATURES[name])):
        if t is ctypes.c_void_p:
            out.append(vals.get(p, 0x10000 * (i + 1)))
        else:
            out.append(vals.get(p, 0))
    return out


def _gemm_rejections(name):
    """(label, changes) pairs, each breaking one rule of the entry point `name`."""
    import ctypes
    params = _GEMM_ENTRIES[name].split()
    has = set(params).__contains__
    wgrad = name.startswith("t2s_wgrad_gemm")
    fold = "fold_A" in params
    v = []
    for i, (p, t) in enumerate(zip(params, _lib.SIGNATURES[name])):
        if t is ctypes.c_void_p:
            if p not in _NULL_ALLOWED:
                v.append(("NULL " + p, {p: None}))
            if p not in _UNALIGNED_ALLOWED:
                v.append(("unaligned " + p, {p: 0x10000 * (i + 1) + 8}))
    v += [("B = 0", dict(B=0)), ("L = 0", dict(L=0)), ("C = 0", dict(C=0)), ("C % 4", dict(C=62)),
          ("Mpad % 256", dict(Mpad=300)), ("Mpad = 0", dict(Mpad=0))]
    # Mpad one tile short of the packed rows: the gate packs 128-channel halves into 256-row tiles, the others are plain rows
    if has("n_res"):
        v.append(("Mpad too small", dict(C=192, n_res=192)))           # needs 384
        v.append(("n_res neither 0 nor C", dict(n_res=32)))
    elif "gate" in name and not name.endswith("dgrad"):
        v.append(("Mpad too small", dict(C=144)))                      # needs 2 x 256
    else:
        v.append(("Mpad too small", dict(C=320)))
    if wgrad:
        v += [("Npad one tile too large", dict(Lp=768)), ("n_tchunks = 0", dict(n_tchunks=0, k1=0)), ("k0 < 0", dict(k0=-1)),
              ("k1 > n_tchunks", dict(k1=4)), ("k0 >= k1", dict(k0=3))]
    else:
        v.append(("Lp one tile too large", dict(Lp=520 + 256)))
    if has("taps"):
        v += [("even taps", dict(taps=2)), ("taps = 0", dict(taps=0)), ("dilation = 0", dict(dilation=0)),
              ("(taps / 2) * dilation > halo", dict(dilation=5))]
    if has("Cin"):
        v.append(("Cin = 0", dict(Cin=0)))
    if fold:
        v.append(("C % 16", dict(C=72)))
    if has("pair8"):
        v.append(("pair8 with C % 32", dict(C=80, pair8=1)))
    if has("act_bchunks"):
        v.append(("act_bchunks below C / 32", dict(act_bchunks=1)))
    if has("x_bchunks"):
        v.append(("x_bchunks below Cin / 32", dict(x_bchunks=1)))
    if name == "t2s_wg_in_win_gate_fold":
        v += [("win_chunks = 3", dict(win_chunks=3)), ("n_cond = 0", dict(n_cond=0)), ("halo < 0", dict(halo=-1, Lp=510))]
    if name == "t2s_wg_in_melwin_gate_fold":
        v += [("K2 % 32", dict(K2=48)), ("K2 = 0", dict(K2=0)), ("P = 0", dict(P=0)), ("Fp below the frames", dict(Fp=74)),
              ("128-row tile shape", dict(C=64))]
    if name == "t2s_conv_bias_act":
        v += [("act = -1", dict(act=-1)), ("act = 3", dict(act=3)), ("no output at all", dict(O_hi=None, O_lo=None, out_f32=None))]
    if name == "t2s_wg_skip_sum":
        v.append(("n_k_chunks = 0", dict(n_k_chunks=0)))
    if name == "t2s_wg_bwd_gate_dgrad":
        v += [("C % 32", dict(C=80)), ("dp_bchunks below 2 C / 32", dict(dp_bchunks=3)), ("tg_bchunks below C / 32", dict(tg_bchunks=1))]
    if name in ("t2s_wg_bwd_gate_dgrad", "t2s_conv_accumulate"):
        v.append(("pair8 on a grid too small for the 256-row kernel", dict(pair8=1)))
    if name == "t2s_wgrad_gemm":
        v += [("ksplit = 17", dict(ksplit=17)), ("ksplit = 0", dict(ksplit=0))]
    if name == "t2s_wgrad_gemm_flat":
        v += [("nsplit larger than the K-steps", dict(nsplit=7)), ("nsplit = 0", dict(nsplit=0)),
              ("a slab without a K-step", dict(nsplit=5))]
    return v


def test_gemm_entry_points_reject_bad_arguments(lib):
    """Every conv-GEMM entry point returns T2S_EINVAL for a valid argument tuple with one rule broken.  The pointers are made up, so
    this runs only where there is no device: a tuple accepted by mistake fails there as a HIP error and reaches no GPU.  The valid
    tuple itself is never called (it would launch)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("made-up pointers: only on a machine without a GPU")
    assert lib.t2s_plane_rows(_GEMM_BASE["L"], _GEMM_BASE["halo"]) == _GEMM_BASE["Lp"]
    assert len(_GEMM_ENTRIES) == 16
    n = 0
    for name in _GEMM_ENTRIES:
        fn = getattr(lib, name)
        for label, changes in _gemm_rejections(name):
            assert fn(*_gemm_args(name, **changes)) == -1, "%s accepted: %s" % (name, label)
            n += 1
    assert n > 400
