"""Helpers of tests/test_longform_gpu.py: the small models, and gate thresholds chosen from the chunks' solo gate trajectories."""
import torch

import streaming_ref as R
from text2speech_amd import longform as L, synth
from text2speech_amd.text import text_to_sequence

DEV = "cuda:0"
HP = synth.TACOTRON_HPARAMS
CFG = R.CFG                                         # synth.WAVEGLOW_SMALL: 64 channels
N_STEPS = 40
SEED = 20240611
SIGMA = 0.666
# Five chunks of 8, 7, 6, 5 and 6 ids (the text's order is not the sorted one), found by a search over short syllable strings: with
# the synthetic weights most texts' gate falls from its first step on, these rise - to five different stop steps under one threshold
CHUNKS = ["티추타.", "토우로", "사추!", "돈!", "푸푸!"]
MIN_FRAMES = 3                                      # a Denoiser refuses an entry of at most 512 samples: 3 frames are 768


def chunk_ids():
    return [torch.from_numpy(text_to_sequence(c)).to(torch.int64)[None] for c in CHUNKS]


def tacotron():
    from text2speech_amd.tacotron import Tacotron
    m = Tacotron(HP, 80, num_speakers=2)
    m.load_state_dict(synth.tacotron_state(), strict=True)
    return m.to(DEV).eval()


def waveglow(half=False):
    from text2speech_amd.glow import WaveGlow
    m = WaveGlow(**CFG)
    m.load_state_dict(synth.waveglow_state(CFG, **R.STRESS), strict=True)
    m = m.to(DEV).eval()
    if half:            # as the reference's inference script: .half() with the 1x1 convolutions put back to float
        m.half()
        for c in m.convinv:
            c.float()
    return m


def set_decoder(model, thr, n):
    model.decoder.gate_threshold, model.decoder.max_decoder_steps = thr, n


def restore_decoder(model):
    set_decoder(model, HP["gate_threshold"], HP["max_decoder_steps"])


def solo_gate_probs(model, seeds):
    """sigmoid(gate) of every chunk decoded alone for N_STEPS frames with its own seed (threshold 2: it never stops)"""
    try:
        set_decoder(model, 2.0, N_STEPS)
        return [torch.sigmoid(model.inference(ids.to(DEV), None, seed=s)[2][0, :, 0].double().cpu())
                for ids, s in zip(chunk_ids(), seeds)]
    finally:
        restore_decoder(model)


def _stops(p, thr):
    above = (p > thr).nonzero()
    return int(above[0]) if above.numel() else p.numel()


def _candidates(probs, margin):
    """(threshold, stop steps) for every gap between two neighbouring values of the trajectories - between them no stop step
    changes - whose nearest values among the entries' prefixes (up to and including the stop step) lie more than `margin` away
    from the threshold, which goes half-way between those: tests/test_batch_inference_gpu.py's method"""
    vals = sorted({float(v) for p in probs for v in p})
    for lo, hi in zip(vals, vals[1:]):
        mid = 0.5 * (lo + hi)
        stops = [_stops(p, mid) for p in probs]
        near = torch.cat([p[:s + 1] for p, s in zip(probs, stops)])
        below, above = near[near < mid], near[near > mid]
        if below.numel() == 0 or above.numel() == 0:
            continue
        lo2, hi2 = float(below.max()), float(above.min())
        if hi2 - lo2 > 2 * margin:
            yield 0.5 * (lo2 + hi2), stops


def pick_threshold(probs, margin=1e-4):
    """A threshold at which every chunk stops before the last step, none in fewer than MIN_FRAMES frames, and at as many different
    steps as can be had (two at least) -> (threshold, stop steps).  Fails where there is none: the tests must not pass vacuously."""
    n = probs[0].numel()
    best, best_key = None, None
    for thr, stops in _candidates(probs, margin):
        if max(stops) >= n - 1 or min(stops) + 1 < MIN_FRAMES:
            continue
        key = (len(set(stops)), -max(stops))
        if best_key is None or key > best_key:
            best, best_key = (thr, stops), key
    assert best is not None and best_key[0] >= 2, ("no gate threshold separates the chunks' stop steps",
                                                   [[round(float(v), 5) for v in p[:12]] for p in probs])
    return best


def pick_truncating_threshold(probs, margin=1e-4):
    """A threshold that exactly one chunk never reaches while every other stops (after MIN_FRAMES frames at least)
    -> (threshold, stop steps, the chunk that runs into max_decoder_steps)"""
    n = probs[0].numel()
    for thr, stops in sorted(_candidates(probs, margin), key=lambda c: -c[0]):
        late = [i for i, s in enumerate(stops) if s >= n]
        if len(late) == 1 and min(stops) + 1 >= MIN_FRAMES:
            return thr, stops, late[0]
    raise AssertionError(("no gate threshold is reached by all chunks but one", [round(float(p.max()), 5) for p in probs]))


def seeds():
    return L.chunk_seeds(SEED, len(CHUNKS))
