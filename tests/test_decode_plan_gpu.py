"""The engine's decode paths at the smallest shapes that reach each kernel chain (16 encoder positions, 4 decoder steps): the plan
the library reports for the struct the engine built (``eng.last_decode_plan``) is the one DESIGN.md section 5b lists for that path,
every optional buffer the engine offered is one the plan uses (no silent fallback), and the outputs are finite.  The plan table
itself is pinned without a GPU in tests/test_decode_plan_cpu.py."""
import pytest
import torch

from text2speech_amd import _lib, synth
from text2speech_amd.tacotron.tacotron import PLAN_USES, DecodePlan, _PLAN_FLAGS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HP = synth.TACOTRON_HPARAMS
T_IN, N = 16, 4


def flags(*names, units=4):
    return DecodePlan(**dict({k: k in names for k in _PLAN_FLAGS}, units=units))


STREAMED = flags("fused_att", "q_parts", "stream_gates", "fold_pre2", "use_ploc", "proj_fused")
FUSED = flags("fused_att", "q_parts", "proj_fused")
BIG = flags("q_big", "one", "proj_fused")
TEACHER_BIG = ("split", "paced", "sig_by_kernel", "q_big", "one")


def _model(train):
    assert torch.cuda.is_available()
    _lib.load()
    from text2speech_amd.tacotron import Tacotron
    m = Tacotron(HP, 80, num_speakers=2)
    m.load_state_dict(synth.tacotron_state(), strict=True)
    m = m.to(DEV)
    return m.train() if train else m.eval()


@pytest.fixture(scope="module")
def model():
    return _model(False)


def _batch(B, seed):
    gen = torch.Generator().manual_seed(seed)
    text = torch.randint(2, 80, (B, T_IN), generator=gen).to(DEV)
    mel = torch.randn(B, 80, N, generator=gen).to(DEV)
    pm = (torch.rand(N + 1, B, 2, 256, generator=gen) < 0.5).to(torch.uint8)
    full = lambda v: torch.full((B,), v, dtype=torch.long, device=DEV)
    return text, pm, (text, full(T_IN), mel, T_IN, torch.zeros(B, device=DEV), full(N))


def _check(eng, want, offered, outputs):
    assert eng.last_decode_plan == want
    assert sorted(eng.last_decode_offer) == sorted(offered)
    for name in eng.last_decode_offer:
        assert any(getattr(eng.last_decode_plan, f) for f in PLAN_USES[name]), "%s offered, not used" % name
    for t in outputs:
        assert bool(torch.isfinite(t).all())
    eng.check_lstm_xbuf()


@pytest.mark.parametrize("B,want,offered", [(1, STREAMED, ["q_part", "gate_part", "ploc", "w_pre2T"]), (5, FUSED, ["q_part"]),
                                            (9, BIG, ["q_part", "att_xbuf"])])
def test_inference_plans(model, B, want, offered):
    text, pm, _ = _batch(B, 100 + B)
    model.decoder.gate_threshold, model.decoder.max_decoder_steps = 2.0, N
    try:
        out = model.inference(text, None, prenet_masks=pm[:N])
    finally:
        model.decoder.gate_threshold, model.decoder.max_decoder_steps = HP["gate_threshold"], HP["max_decoder_steps"]
    assert tuple(out[0].shape) == (B, 80, N) and tuple(out[3].shape) == (B, N, T_IN)
    _check(model._eng(), want, offered, out)


def test_no_grad_forward_9_items_plan(model):
    _, pm, inp = _batch(9, 209)
    with torch.no_grad():
        out = model(inp, prenet_masks=pm)
    _check(model._eng(), flags(*TEACHER_BIG), ["q_part", "att_xbuf", "pace_flag"], out)


@pytest.mark.parametrize("B,want,offered", [(2, flags("split", "fused_att", "q_parts", units=2), ["q_part"]),
                                            (9, flags(*TEACHER_BIG, units=2), ["q_part", "att_xbuf", "pace_flag"])])
def test_training_forward_plans(B, want, offered):
    m = _model(True)
    _, pm, inp = _batch(B, 400 + B)
    out = m(inp, prenet_masks=pm)
    assert out[0].requires_grad                     # (the path with the per-step saves)
    _check(m._eng(), want, offered, [t.detach() for t in out])


def test_single_step_decode_plan(model):
    dec = model.decoder
    eng = model._eng()
    memory = torch.randn(2, T_IN, 512, generator=torch.Generator().manual_seed(5)).to(DEV)
    dec.initialize_decoder_states(memory, None)
    want = flags("fused_att", "q_parts")
    assert eng.last_decode_plan == want
    outs = []
    for step in range(2):       # both step slots (the h ping-pong): one plan
        x = torch.relu(torch.randn(2, 256, generator=torch.Generator().manual_seed(50 + step))).to(DEV)
        outs += list(dec.decode(x))
    _check(eng, want, ["q_part"], outs)
