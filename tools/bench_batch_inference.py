#!/usr/bin/env python3
"""Tacotron.inference_batch against the same texts run one at a time (synthetic weights, eval mode): B in {1, 2, 4, 8} texts
of different lengths (up to 128 symbols), every one forced to the same frame count (gate threshold 2.0, max_decoder_steps
frames).  Prints one JSON line: per B, ms per call and decoded frames/s of both, and their ratio.  --half: model.half() (the
reference's inference precision: the decode streams fp16 LSTM weights, engine switch decode_w16; --w16-off: the f32 copies);
--batch-only: no solo runs."""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from text2speech_amd import synth  # noqa: E402
from text2speech_amd.tacotron import Tacotron  # noqa: E402

LENGTHS = (128, 117, 106, 95, 84, 73, 62, 51)


def _timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=400)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--half", action="store_true")
    ap.add_argument("--w16-off", action="store_true")
    ap.add_argument("--batch-only", action="store_true")
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 2, 4, 8])
    args = ap.parse_args()
    hp = synth.TACOTRON_HPARAMS
    model = Tacotron(hp, 80, num_speakers=2)
    model.load_state_dict(synth.tacotron_state())
    model = model.cuda().eval()
    if args.half:
        model = model.half()
    if args.w16_off:
        model._eng().decode_w16 = False
    model.decoder.gate_threshold, model.decoder.max_decoder_steps = 2.0, args.frames
    gen = torch.Generator().manual_seed(11)
    out = {"frames_per_text": args.frames, "lengths": list(LENGTHS), "half": args.half}
    with contextlib.redirect_stderr(io.StringIO()):         # (the max-decoder-steps warning of every call)
        for B in args.batches:
            lens = list(LENGTHS[:B])
            ids = torch.randint(2, 80, (B, max(lens)), generator=gen).cuda()
            batch = lambda: model.inference_batch(ids, lens)
            solo = lambda: [model.inference(ids[b:b + 1, :L]) for b, L in enumerate(lens)]
            batch()
            t_batch = _timed(batch, args.reps)
            frames = B * args.frames
            out["B%d" % B] = {"batch_ms": round(t_batch * 1e3, 2), "batch_frames_per_s": round(frames / t_batch),
                              "batch_us_per_step": round(t_batch / args.frames * 1e6, 2),
                              "decode_w16": model._eng().last_decode_w16}
            if args.batch_only:
                continue
            solo()
            t_solo = _timed(solo, args.reps)
            out["B%d" % B].update({"solo_ms": round(t_solo * 1e3, 2), "solo_frames_per_s": round(frames / t_solo),
                                   "speedup": round(t_solo / t_batch, 2)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
