"""Host side of WaveGlow.infer_batch's fp16 chain (engine switch infer_batch_w16): which models are eligible, the decision table of
the two switches, the overflow refusal's wording and the ctypes table of the three _h16_ragged entry points.  No GPU."""
import os
import re

import pytest
import torch

from text2speech_amd import _lib, glow

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAGGED_H16 = ("t2s_wg_start_h16_ragged", "t2s_wg_in_cond_gate_fold_h16_ragged", "t2s_wg_res_only_h16_ragged")


def _model(C=32, half=True):
    m = glow.WaveGlow(n_mel_channels=4, n_flows=2, n_group=8, n_early_every=4, n_early_size=2,
                      WN_config=dict(n_layers=2, n_channels=C, kernel_size=3))
    if half:
        m.half()
        for c in m.convinv:         # the reference script's call order: only the WN parameters count
            c.float()
    return m


def test_w16_batch_eligible():
    """every WN parameter fp16, n_channels % 16 == 0, the shipped library and the three symbols"""
    lib = _lib.load()
    assert _lib.operand_format() == 0 and all(hasattr(lib, n) for n in RAGGED_H16)
    assert glow._Engine._W16_BATCH_SYMBOLS == RAGGED_H16
    assert _model()._eng().w16_batch_eligible() == (True, "")
    ok, why = _model(half=False)._eng().w16_batch_eligible()
    assert not ok and "float16" in why
    mixed = _model()
    mixed.WN[1].res_skip_layers[0].float()
    ok, why = mixed._eng().w16_batch_eligible()
    assert not ok and "float16" in why
    ok, why = _model(C=24)._eng().w16_batch_eligible()
    assert not ok and "16" in why
    # w16_eligible is as it was: infer_batch is not its business
    ok, why = _model()._eng().w16_eligible(batch=True)
    assert not ok and "infer_batch" in why


def test_a_library_without_the_symbols(monkeypatch):
    """an older diagnostic library: not eligible, and the reason names what is missing"""
    real = _lib.load()

    class Old:
        def __getattr__(self, name):
            if name in RAGGED_H16[1:]:
                raise AttributeError(name)
            return getattr(real, name)
    monkeypatch.setattr(_lib, "load", lambda: Old())
    ok, why = _model()._eng().w16_batch_eligible()
    assert not ok and RAGGED_H16[1] in why and RAGGED_H16[2] in why and RAGGED_H16[0] not in why


@pytest.mark.parametrize("infer_w16", [None, False, True])
def test_decision_table(infer_w16):
    """infer_batch_w16 is False by default and None means False: infer_batch is then decided by infer_w16 as before (never the fp16
    chain; a raise under True).  With infer_batch_w16 = True the batch takes the chain whatever infer_w16 says, and infer_w16 keeps
    deciding infer alone."""
    _lib.load()
    eng = _model()._eng()
    assert eng.infer_batch_w16 is False and eng.last_infer_batch_w16 is False
    eng.infer_w16 = infer_w16
    solo = {None: glow._INFER_W16_AUTO, False: False, True: True}[infer_w16]
    for off in (False, None):
        eng.infer_batch_w16 = off
        assert eng.use_batch_w16() is False
        assert eng.use_w16() is solo
        if infer_w16 is True:
            with pytest.raises(_lib.T2SError, match="infer_batch"):
                eng.use_w16(batch=True)
        else:
            assert eng.use_w16(batch=True) is False
    eng.infer_batch_w16 = True
    assert eng.use_batch_w16() is True
    assert eng.use_w16() is solo


def test_required_but_not_eligible():
    """True on an f32 model, on mixed dtypes and on n_channels = 24 raises T2SError naming the switch; nothing was packed"""
    _lib.load()
    mixed = _model()
    mixed.WN[0].in_layers[1].float()
    for m in (_model(half=False), mixed, _model(C=24)):
        eng = m._eng()
        eng.infer_batch_w16 = True
        with pytest.raises(_lib.T2SError, match="infer_batch_w16 = True"):
            eng.use_batch_w16()
        assert eng.packed16 is None and eng.packed is None
        eng.infer_batch_w16 = False
        assert eng.use_batch_w16() is False


def test_refusal_names_the_batch_switch(monkeypatch):
    monkeypatch.delenv("T2S_F16_GUARD", raising=False)
    t = torch.zeros(2, 8)
    glow.WaveGlow._refuse_overflow(t, w16="infer_batch_w16")
    t[0, 5] = float("inf")
    with pytest.raises(_lib.T2SError, match="infer_batch_w16 = False"):
        glow.WaveGlow._refuse_overflow(t, w16="infer_batch_w16")
    with pytest.raises(_lib.T2SError, match=r"\binfer_w16 = False"):
        glow.WaveGlow._refuse_overflow(t, w16=True)


def test_h16_ragged_signatures():
    """Each of the three takes its _h16 partner's argument list with one more pointer, `const int* lengths`, in front of `stream` -
    in the ctypes table, in the loaded library and in include/t2s_hip.h."""
    src = open(os.path.join(ROOT, "include", "t2s_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decl = {name: [a.strip() for a in re.sub(r"\s+", " ", args).split(",")]
            for name, args in re.findall(r"\bint\s+(t2s_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", src)}
    assert sorted(n for n in decl if n.endswith("_h16_ragged")) == sorted(RAGGED_H16)
    lib = _lib.load()
    for n in RAGGED_H16:
        partner = n.replace("_h16_ragged", "_h16")
        assert decl[partner][-1] == "void* stream"
        assert decl[n] == decl[partner][:-1] + ["const int* lengths", "void* stream"], n
        sig, psig = _lib.SIGNATURES[n], _lib.SIGNATURES[partner]
        assert sig == psig[:-1] + [_lib.c_vp, _lib.c_vp] and psig[-1] is _lib.c_vp, n
        assert list(getattr(lib, n).argtypes) == sig
    assert lib.t2s_abi_version() == 4


def test_engine_entry_point_table():
    """The engine's stage table (glow._ENTRY_POINTS: split-bf16, its infer_batch form, the fp16 chain, its infer_batch form): every
    name it can resolve is in the ctypes table; an infer_batch column differs from the column before it only by an entry point
    listed in glow._TAKES_LENGTHS; each of those has its partner's argument list with exactly one more pointer in front of
    `stream`; and a plan hands `lengths` to exactly those.  A typo in the table fails here, without a GPU."""
    table, takes = glow._ENTRY_POINTS, glow._TAKES_LENGTHS
    names = {n for row in table.values() for n in row if n is not None}
    assert names | set(takes.values()) | set(glow._START_TAKES_WINDOW) <= set(_lib.SIGNATURES)
    assert set(takes) <= names and set(RAGGED_H16) <= set(takes)
    for stage, row in table.items():
        assert len(row) == 4 and row[0] is not None, stage
        for plain, batch in ((row[0], row[1]), (row[2], row[3])):
            assert plain not in takes and (batch is None or batch == plain or batch in takes), stage
    for n, partner in takes.items():
        sig, psig = _lib.SIGNATURES[n], _lib.SIGNATURES[partner]
        assert psig[-1] is _lib.c_vp and sig == psig[:-1] + [_lib.c_vp, _lib.c_vp], n
    _lib.load()
    eng = _model()._eng()
    lens = torch.tensor([4, 2], dtype=torch.int32)
    for h16 in (False, True):
        for col, ln in ((2 * h16, None), (2 * h16 + 1, lens)):
            plan = eng._plan(h16, ln)
            assert plan.h16 is h16 and plan.lens is ln and plan.pk is None and plan.melwin is None
            assert plan.path == ((False, False, None) if h16 else eng.path(compose=ln is None)) == eng.last_path
            for stage, row in table.items():
                name, lengths = plan.entry[stage]
                assert name == row[col], (stage, h16)
                assert [a.value for a in lengths] == ([lens.data_ptr()] if name in takes else []), (stage, h16)
    assert eng.packed is None and eng.packed16 is None
