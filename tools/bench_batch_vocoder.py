#!/usr/bin/env python3
"""WaveGlow.infer_batch against the same mels vocoded one at a time (config.json-default WaveGlow, synthetic weights): B in
{1, 2, 4, 8} mels of different lengths.  Per B, in one process, after a warm-up call each and interleaved over the repetitions
(the order rotates from one repetition to the next):
  (a) infer on one mel at a time;
  (b) infer_batch on the padded batch;
  (c) infer on the padded batch - its short entries are wrong; it is what the same grid costs without the masks.
Each has a model of its own, so that none of them re-allocates the one resident workspace shape the others left behind.
Prints one JSON line: per B the median, least and greatest ms per call of each, valid samples/s of (a) and (b) and their ratio, and
(b) - (c) next to (c)'s own spread.  --divide N: every mel N times shorter (short utterances, the grids that do not fill the chip).
--half: the models are .half() with the 1x1 convolutions float (the reference script's call order): (a) and (c) then run on the fp16
chain wherever infer_w16 = None selects it, and --w16 on | off sets infer_batch_w16 for (b) - on: the fp16 chain whose GEMMs skip
the column tiles behind an entry's end, off (default): split-bf16 planes, the padding computed.  One setting per process, so that
settings and libraries (T2S_LIB_PATH) can alternate on one box.  With --half the overflow guard's read-back per call is switched
off for the timed calls (T2S_F16_GUARD=0) after the warm-up calls were checked with it on.  Per B also the share of the gate GEMM's
column tiles that lie wholly behind their entry's end (what --w16 on skips)."""
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
from text2speech_amd.glow import WaveGlow  # noqa: E402

FRAMES = (400, 372, 344, 301, 268, 233, 187, 150)
SIGMA = 0.666


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
    ap.add_argument("--half", action="store_true", help=".half() models (1x1 convolutions float)")
    ap.add_argument("--w16", choices=("off", "on"), default="off", help="infer_batch_w16 of the batched model (needs --half)")
    args = ap.parse_args()
    if args.w16 == "on" and not args.half:
        ap.error("--w16 on needs --half")
    all_frames = [max(1, f // args.divide) for f in FRAMES]
    cfg = synth.WAVEGLOW_DEFAULT
    sd = synth.waveglow_state(cfg)
    models = []
    for _ in range(3):
        m = WaveGlow(**cfg)
        m.load_state_dict(sd)
        m = m.cuda().eval()
        if args.half:
            m.half()
            for c in m.convinv:
                c.float()
        models.append(m)
    models[1]._eng().infer_batch_w16 = args.w16 == "on"
    gen = torch.Generator().manual_seed(17)
    out = {"frames": all_frames, "reps": args.reps, "sigma": SIGMA, "half": args.half, "infer_batch_w16": args.w16 == "on",
           "lib": os.environ.get("T2S_LIB_PATH", "shipped")}
    cols_per_frame = models[0].upsample.stride[0] // cfg["n_group"]
    for B in (1, 2, 4, 8):
        frames = all_frames[:B]
        mel = torch.randn(B, 80, max(frames), generator=gen).cuda()
        solo_mels = [mel[b:b + 1, :, :f].contiguous() for b, f in enumerate(frames)]
        lens = torch.tensor(frames)
        runs = {
            "solo": lambda: [models[0].infer(x, sigma=SIGMA) for x in solo_mels],
            "batch": lambda: models[1].infer_batch(mel, lens, sigma=SIGMA),
            "padded": lambda: models[2].infer(mel, sigma=SIGMA),
        }
        os.environ.pop("T2S_F16_GUARD", None)
        for fn in runs.values():            # warm-up: packs the weights, sizes the workspace, and checks the audio with the guard on
            fn()
        paths = {"solo_w16": models[0]._eng().last_infer_w16, "batch_w16": models[1]._eng().last_infer_batch_w16,
                 "padded_w16": models[2]._eng().last_infer_w16}
        if args.half:
            os.environ["T2S_F16_GUARD"] = "0"
        ntiles = -(-max(frames) * cols_per_frame // 256)
        skipped = sum(ntiles - -(-f * cols_per_frame // 256) for f in frames)
        ms = {k: [] for k in runs}
        order = list(runs)
        for r in range(args.reps):          # rotated: each of the three follows each of the others equally often
            for k in order[r % 3:] + order[:r % 3]:
                ms[k].append(_once(runs[k]))
        st = {k: _stats(v) for k, v in ms.items()}
        valid = 256 * sum(frames)
        out["B%d" % B] = {
            "solo": st["solo"], "batch": st["batch"], "padded": st["padded"],
            "solo_valid_samples_per_s": round(valid / st["solo"]["median_ms"] * 1e3),
            "batch_valid_samples_per_s": round(valid / st["batch"]["median_ms"] * 1e3),
            "speedup": round(st["solo"]["median_ms"] / st["batch"]["median_ms"], 2),
            "batch_minus_padded_ms": round(st["batch"]["median_ms"] - st["padded"]["median_ms"], 3),
            "padded_spread_ms": round(st["padded"]["max_ms"] - st["padded"]["min_ms"], 3),
            "gate_tiles_behind_the_end": round(skipped / (ntiles * B), 4),
            **paths,
        }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
