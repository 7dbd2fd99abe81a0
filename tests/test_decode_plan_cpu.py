"""The Tacotron decode driver's plan (``t2s_taco_decode_plan``, host only) against a table written from the driver's rules: which
kernel chain ``t2s_taco_decode_steps`` follows for a decoder struct.  The pointers are made up (distinct, 256-byte aligned, never
dereferenced); no GPU is needed.  The streamed-gate rows depend on the device's CU count: the library takes 256 where no device
answers, which is also what the MI355X reports."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

from text2speech_amd import _lib, build
from text2speech_amd.tacotron.tacotron import DecodePlan, _DecoderStruct, _PLAN_FLAGS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = D = 1024
P, E, N_MEL, T_CAP = 256, 512, 80, 64

REQUIRED = ["att_w_ih", "att_w_hh", "att_b_ih", "att_b_hh", "dec_w_ih", "dec_w_hh", "dec_b_ih", "dec_b_hh", "w_query", "w_loc_conv",
            "w_loc_dense", "w_v", "w_loc_denseT", "memory", "pmem", "att_h0", "att_h1", "att_c", "dec_h0", "dec_h1", "dec_c", "att_w",
            "att_wcum", "ctx", "q", "energies", "align_out"]
TEACHER = ["pre_all", "hc_all"]
FREE = ["w_proj", "b_proj", "w_pre2", "pre1", "pre2", "mel_gate_out", "prenet_masks"]
SAVES = ["att_gates_all", "att_c_all", "dec_gates_all", "dec_c_all", "att_h_all", "q_all", "wcum_all"]
STREAM = ["gate_part", "ploc", "w_pre2T"]
ALL_OPTIONAL = STREAM + ["q_part", "att_xbuf", "pace_flag"]


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def struct(B, T_in, teacher, given=(), **fields):
    """A t2s_taco_decoder at the default dimensions with every required pointer and those named in `given`; `fields` overrides."""
    d = _DecoderStruct()
    dims = dict(B=B, T_in=T_in, n_mel=N_MEL, prenet_dim=P, enc_dim=E, att_rnn_dim=A, dec_rnn_dim=D, att_dim=128, loc_filters=32,
                loc_kernel=31, T_cap=T_CAP, teacher_forced=int(teacher), mask_steps=0 if teacher else T_CAP)
    for k, v in dims.items():
        setattr(d, k, v)
    names = REQUIRED + (TEACHER if teacher else FREE) + list(given)
    for i, name in enumerate(names):
        setattr(d, name, 0x10000000 + 0x1000000 * i)
    if not teacher:     # one row block [n_mel + 1 | prenet] as the engine packs it
        d.w_projpre = d.w_proj + 4 * (N_MEL + 1) * (D + E)
        d.b_projpre = d.b_proj + 4 * (N_MEL + 1)
    d.att_drop_scale = d.dec_drop_scale = 1.0
    for k, v in fields.items():
        setattr(d, k, v)
    return d


def plan(lib, d, step0=0, n_steps=4):
    bits = ctypes.c_uint(0xFFFFFFFF)
    rc = lib.t2s_taco_decode_plan(ctypes.byref(d), step0, n_steps, ctypes.byref(bits))
    return rc, (DecodePlan.from_bits(bits.value) if rc == 0 else None)


def flags(*names, units=4):
    return DecodePlan(**dict({k: k in names for k in _PLAN_FLAGS}, units=units))


FUSED = ("fused_att", "q_parts", "proj_fused")                          # the plain small-batch chain
STREAMED = FUSED + ("stream_gates", "fold_pre2", "use_ploc")            # ... with the streamed gates and what rides on them
TEACHER_BIG = ("split", "paced", "sig_by_kernel", "q_big", "one")       # teacher-forced at 9+ items with everything offered


def test_plan_bits_match_the_header():
    src = open(os.path.join(ROOT, "include", "t2s_hip.h")).read()
    bits = [(m.group(1).lower(), int(m.group(2), 16)) for m in re.finditer(r"#define T2S_PLAN_(\w+) (0x[0-9a-fA-F]+)u", src)]
    assert bits == [(name, 1 << i) for i, name in enumerate(_PLAN_FLAGS + ("units_2",))]


@pytest.mark.parametrize("B", [1, 4])
def test_autoregressive_up_to_4_items_streams_gates(lib, B):
    assert plan(lib, struct(B, 48, False, ALL_OPTIONAL)) == (0, flags(*STREAMED))


@pytest.mark.parametrize("B", [5, 8])
def test_autoregressive_5_to_8_items_ignores_the_stream_buffers(lib, B):
    assert plan(lib, struct(B, 48, False, ALL_OPTIONAL)) == (0, flags(*FUSED))


def test_autoregressive_without_gate_part_is_the_plain_fused_chain(lib):
    assert plan(lib, struct(1, 48, False, ["q_part", "ploc", "w_pre2T"])) == (0, flags(*FUSED))
    assert plan(lib, struct(1, 48, False, ["ploc", "w_pre2T"])) == (0, flags("fused_att", "proj_fused"))     # no q_part either


def test_autoregressive_past_512_positions_is_three_launches_with_the_query_gemv(lib):
    assert plan(lib, struct(1, 513, False, ALL_OPTIONAL)) == (0, flags("proj_fused"))
    assert plan(lib, struct(1, 512, False, ALL_OPTIONAL)) == (0, flags(*STREAMED))


def test_autoregressive_9_items_sums_partial_queries_in_one_launch_energies(lib):
    assert plan(lib, struct(9, 70, False, ["q_part", "att_xbuf"])) == (0, flags("q_big", "one", "proj_fused"))
    assert plan(lib, struct(9, 70, False, ["q_part"])) == (0, flags("q_big", "proj_fused"))
    assert plan(lib, struct(9, 70, False, ["att_xbuf"])) == (0, flags("one", "proj_fused"))


def test_teacher_forced_12_items_with_saves(lib):
    given = SAVES + ["q_part", "att_xbuf", "pace_flag"]
    assert plan(lib, struct(12, 30, True, given)) == (0, flags(*TEACHER_BIG, units=2))
    assert plan(lib, struct(12, 600, True, given)) == (0, flags("split", "paced", "sig_by_kernel", "q_big", units=2))
    assert plan(lib, struct(12, 30, True, SAVES + ["q_part", "att_xbuf"])) == (0, flags("split", "q_big", "one", units=2))
    # the no-grad forward at 9+ items: att_h_all is the only save
    assert plan(lib, struct(12, 30, True, ["att_h_all", "q_part", "att_xbuf", "pace_flag"])) == (0, flags(*TEACHER_BIG))
    # a pace word that is not 8-byte aligned: chunks
    d = struct(12, 30, True, given)
    d.pace_flag += 4
    assert plan(lib, d) == (0, flags("split", "q_big", "one", units=2))


def test_teacher_forced_12_items_unpaced_by_environment(lib):
    """T2S_DECODE_PACED is read once per process: a child."""
    code = ("import sys; sys.path.insert(0, %r); import tests.test_decode_plan_cpu as t; from text2speech_amd import _lib\n"
            "rc, p = t.plan(_lib.load(), t.struct(12, 30, True, t.SAVES + ['q_part', 'att_xbuf', 'pace_flag']))\n"
            "assert rc == 0 and p == t.flags('split', 'q_big', 'one', units=2), p") % ROOT
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, T2S_DECODE_PACED="0"), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_teacher_forced_small_batch(lib):
    assert plan(lib, struct(3, 30, True, SAVES + ["q_part"])) == (0, flags("split", "fused_att", "q_parts", units=2))
    # Decoder.decode: single steps without att_h_all - serial; odd and even step slots follow one plan
    d = struct(2, 30, True, ["q_part"])
    assert plan(lib, d, 0, 1) == plan(lib, d, 1, 1) == (0, flags("fused_att", "q_parts"))


def test_attention_dim_64_does_not_stream(lib):
    assert plan(lib, struct(1, 48, False, ALL_OPTIONAL, att_dim=64)) == (0, flags(*FUSED))


def test_projection_rows_apart_are_two_launches(lib):
    d = struct(1, 48, False, ALL_OPTIONAL)
    d.w_projpre += 256
    assert plan(lib, d) == (0, flags(*[f for f in STREAMED if f != "proj_fused"]))
    d = struct(1, 48, False, ALL_OPTIONAL)
    d.b_projpre += 4
    assert plan(lib, d) == (0, flags(*[f for f in STREAMED if f != "proj_fused"]))


def test_plan_rejects_what_the_decode_call_rejects(lib):
    ok = lambda **kw: struct(1, 48, False, ALL_OPTIONAL, **kw)
    assert plan(lib, ok())[0] == 0
    assert lib.t2s_taco_decode_plan(ctypes.byref(ok()), 0, 4, None) == 0            # bits may be NULL
    assert lib.t2s_taco_decode_plan(None, 0, 4, None) == -1
    for label, d, step0, n in [("even loc_kernel", ok(loc_kernel=30), 0, 4), ("A != D", ok(dec_rnn_dim=512), 0, 4),
                               ("past T_cap", ok(), T_CAP - 3, 4), ("step0 < 0", ok(), -1, 4), ("n_steps = 0", ok(), 0, 0),
                               ("B = 0", struct(0, 48, False, ALL_OPTIONAL), 0, 4), ("attention dim 129", ok(att_dim=129), 0, 4),
                               ("33 filters", ok(loc_filters=33), 0, 4), ("prenet_dim % 4", ok(prenet_dim=254), 0, 4)]:
        assert plan(lib, d, step0, n) == (-1, None), label
    assert plan(lib, ok(), T_CAP - 4, 4)[0] == 0
    for name in REQUIRED + FREE + ["w_projpre", "b_projpre"]:
        if name in ("att_b_ih", "att_b_hh", "dec_b_ih", "dec_b_hh", "w_loc_denseT"):        # optional in the ABI
            continue
        assert plan(lib, ok(**{name: None})) == (-1, None), name
    for name in TEACHER:
        assert plan(lib, struct(12, 30, True, SAVES, **{name: None})) == (-1, None), name
