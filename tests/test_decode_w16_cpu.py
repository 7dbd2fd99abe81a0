"""The fp16-weight decode entry points on the host: ``t2s_taco_decode_plan_w16`` accepts what ``t2s_taco_decode_steps_w16`` runs,
reports the plan of ``t2s_taco_decode_plan`` and the LSTM bytes one step reads, and refuses what the fp16 kernels do not cover.  The
pointers are made up (distinct, 256-byte aligned, never dereferenced); no GPU is needed."""
import ctypes

import pytest

from test_decode_plan_cpu import A, ALL_OPTIONAL, D, E, P, SAVES, struct
from text2speech_amd import _lib, build

EINVAL = -1
MEMBERS = ("att_w_ih", "att_w_hh", "dec_w_ih", "dec_w_hh")
ELEMS = 4 * A * (P + E + A) + 4 * D * (A + E + D)


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def w16(**fields):
    w = _lib.TacoW16()
    for i, name in enumerate(MEMBERS):
        setattr(w, name, 0x60000000 + 0x1000000 * i)
    for k, v in fields.items():
        setattr(w, k, v)
    return w


def plan16(lib, d, w, step0=0, n_steps=4):
    bits, nbytes = ctypes.c_uint(0xFFFFFFFF), ctypes.c_longlong(-1)
    rc = lib.t2s_taco_decode_plan_w16(ctypes.byref(d), None if w is None else ctypes.byref(w), step0, n_steps, ctypes.byref(bits),
                                      ctypes.byref(nbytes))
    return rc, bits.value, nbytes.value


def plan32(lib, d, step0=0, n_steps=4):
    bits = ctypes.c_uint(0xFFFFFFFF)
    assert lib.t2s_taco_decode_plan(ctypes.byref(d), step0, n_steps, ctypes.byref(bits)) == 0
    return bits.value


def small(B, given=ALL_OPTIONAL, **kw):
    """The small sizes of the decode tests: P 32, E 64, A = D 128."""
    d = struct(B, 40, False, given, prenet_dim=32, enc_dim=64, att_rnn_dim=128, dec_rnn_dim=128, n_mel=20, **kw)
    d.w_projpre = d.w_proj + 4 * 21 * (128 + 64)
    d.b_projpre = d.b_proj + 4 * 21
    return d


def test_element_count_of_the_reference_sizes():
    assert ELEMS == 4096 * 4352


@pytest.mark.parametrize("B", [1, 4, 5, 8])
def test_accepts_autoregressive_reference_sizes(lib, B):
    d = struct(B, 48, False, ALL_OPTIONAL)
    rc, bits, nbytes = plan16(lib, d, w16())
    assert rc == 0
    assert bits == plan32(lib, d)
    assert nbytes == 35_651_584 == 2 * ELEMS
    rc, bits, nbytes = plan16(lib, d, None)
    assert (rc, bits, nbytes) == (0, plan32(lib, d), 71_303_168)
    assert nbytes == 4 * ELEMS


def test_accepts_small_sizes(lib):
    d = small(3)
    rc, bits, nbytes = plan16(lib, d, w16())
    assert (rc, bits) == (0, plan32(lib, d))
    assert nbytes == 2 * (4 * 128 * (32 + 64 + 128) + 4 * 128 * (128 + 64 + 128))


def test_outputs_may_be_null(lib):
    d = struct(1, 48, False, ALL_OPTIONAL)
    assert lib.t2s_taco_decode_plan_w16(ctypes.byref(d), ctypes.byref(w16()), 0, 4, None, None) == 0


def test_without_w_every_struct_of_the_f32_plan_is_accepted(lib):
    """w = NULL reports the f32 figure for what t2s_taco_decode_plan accepts: teacher forced, 9+ items, saves."""
    for d in (struct(12, 30, True, SAVES + ["q_part", "att_xbuf", "pace_flag"]), struct(9, 70, False, ["q_part", "att_xbuf"]),
              struct(3, 30, True, SAVES + ["q_part"])):
        assert plan16(lib, d, None) == (0, plan32(lib, d), 4 * ELEMS)
    assert plan16(lib, struct(1, 48, False, ALL_OPTIONAL, loc_kernel=30), None)[0] == EINVAL


def test_refusals(lib):
    ok = lambda **kw: struct(1, 48, False, ALL_OPTIONAL, **kw)
    assert plan16(lib, ok(), w16())[0] == 0
    assert plan16(lib, struct(3, 30, True, ["q_part"]), w16())[0] == EINVAL, "teacher forced"
    assert plan16(lib, struct(9, 48, False, ALL_OPTIONAL), w16())[0] == EINVAL, "B = 9"
    assert plan16(lib, struct(8, 48, False, ALL_OPTIONAL), w16())[0] == 0
    for name in SAVES:
        assert plan16(lib, ok(**{name: 0x7F000000}), w16())[0] == EINVAL, name
    for name in MEMBERS:
        assert plan16(lib, ok(), w16(**{name: None}))[0] == EINVAL, name + " NULL"
        w = w16()
        setattr(w, name, getattr(w, name) + 4)
        assert plan16(lib, ok(), w)[0] == EINVAL, name + " + 4 bytes"
        setattr(w, name, getattr(w, name) + 4)
        assert plan16(lib, ok(), w)[0] == 0, name + " + 8 bytes"
    # what the f32 validation refuses is refused here too, the f32 matrix pointers of `d` included
    assert plan16(lib, ok(att_w_ih=None), w16())[0] == EINVAL
    assert plan16(lib, ok(), w16(), 62, 4)[0] == EINVAL
    assert lib.t2s_taco_decode_plan_w16(None, ctypes.byref(w16()), 0, 4, None, None) == EINVAL
    # the steps call validates before it touches a stream or a pointer: the same answers, and NULL `w` is refused there
    for d, w in ((struct(9, 48, False, ALL_OPTIONAL), w16()), (struct(3, 30, True, ["q_part"]), w16()), (ok(), w16(dec_w_hh=None)),
                 (ok(att_gates_all=0x7F000000), w16())):
        assert lib.t2s_taco_decode_steps_w16(ctypes.byref(d), ctypes.byref(w), 0, 4, None) == EINVAL
    assert lib.t2s_taco_decode_steps_w16(ctypes.byref(ok()), None, 0, 4, None) == EINVAL


def test_abi_is_still_version_4(lib):
    assert lib.t2s_abi_version() == 4
    assert lib.t2s_sizeof_taco_decoder() == ctypes.sizeof(type(struct(1, 48, False)))
    assert ctypes.sizeof(_lib.TacoW16) == 4 * ctypes.sizeof(ctypes.c_void_p)
    for name in ("t2s_taco_decode_steps_w16", "t2s_taco_decode_plan_w16"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
