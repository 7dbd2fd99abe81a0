#!/usr/bin/env python3
"""The back end of a served batch - Denoiser, then int16 PCM - on WaveGlow.infer_batch's padded audio, against the same entries
processed one at a time (config.json-default WaveGlow, synthetic weights; the mels of tools/bench_batch_vocoder.py: FRAMES x 256
samples, B in {1, 2, 4, 8}).  Per B, in one process, after a warm-up call each and interleaved over the repetitions (the order rotates
from one repetition to the next), synchronised around each call:
  (a) Denoiser.forward + to_pcm16 on one entry's slice at a time;
  (b) Denoiser.denoise_batch + to_pcm16(lengths) on the padded batch;
  (c) infer_batch alone on the same batch: what share of a served batch the back end is.
Prints one JSON line: per B the median, least and greatest ms per call of each, (a) / (b), and (b) / ((b) + (c)).
--divide N: every mel N times shorter."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from text2speech_amd import synth  # noqa: E402
from text2speech_amd.audio import Denoiser, to_pcm16  # noqa: E402
from text2speech_amd.glow import WaveGlow  # noqa: E402

FRAMES = (400, 372, 344, 301, 268, 233, 187, 150)
SIGMA = 0.666
STRENGTH = 0.1


def _once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _stats(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--divide", type=int, default=1, help="every mel this many times shorter")
    args = ap.parse_args()
    all_frames = [max(3, f // args.divide) for f in FRAMES]          # (3 frames = 768 samples: more than the Denoiser's n_fft / 2)
    cfg = synth.WAVEGLOW_DEFAULT
    m = WaveGlow(**cfg)
    m.load_state_dict(synth.waveglow_state(cfg))
    m = m.cuda().eval()
    dn = Denoiser(m).cuda()
    gen = torch.Generator().manual_seed(17)
    out = {"frames": all_frames, "reps": args.reps, "sigma": SIGMA, "strength": STRENGTH, "lib": os.environ.get("T2S_LIB_PATH", "shipped")}
    for B in (1, 2, 4, 8):
        frames = all_frames[:B]
        mel = torch.randn(B, 80, max(frames), generator=gen).cuda()
        lens = torch.tensor(frames)
        audio, alen = m.infer_batch(mel, lens, sigma=SIGMA)
        slices = [audio[b:b + 1, :256 * f].contiguous() for b, f in enumerate(frames)]
        runs = {
            "solo": lambda: [to_pcm16(dn(x, strength=STRENGTH)) for x in slices],
            "batch": lambda: to_pcm16(*dn.denoise_batch(audio, alen, STRENGTH)),
            "infer_batch": lambda: m.infer_batch(mel, lens, sigma=SIGMA),
        }
        for fn in runs.values():
            fn()
        ms = {k: [] for k in runs}
        order = list(runs)
        for r in range(args.reps):          # rotated: each of the three follows each of the others equally often
            for k in order[r % 3:] + order[:r % 3]:
                ms[k].append(_once(runs[k]))
        st = {k: _stats(v) for k, v in ms.items()}
        out["B%d" % B] = {
            **st,
            "solo_over_batch": round(st["solo"]["median_ms"] / st["batch"]["median_ms"], 2),
            "back_end_share_of_served_batch": round(st["batch"]["median_ms"] / (st["batch"]["median_ms"] + st["infer_batch"]["median_ms"]), 4),
        }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
