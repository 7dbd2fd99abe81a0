#!/usr/bin/env python3
"""WaveGlow.infer of a .half() model on one MI355X, the reference's inference precision (inference.py:59-74): 512 channels, B = 1,
1000 and 200 mel frames, sigma 0.666.  The engine switch infer_w16 decides whether the call runs on fp16 planes with one-plane
weights (two MFMA products per MAC) or on split-bf16: by default whatever `None` selects, --w16-on requires the fp16 chain,
--w16-off forbids it.  --float: the same on an f32 model (never the fp16 chain).

Prints one JSON line: ms per call (mean and min of --reps timed calls after one warm-up call, weights already packed) per length,
and what ran.  T2S_F16_GUARD=0 is set for the timed calls: the overflow check is a device read-back per call."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from text2speech_amd import synth  # noqa: E402
from text2speech_amd.glow import WaveGlow  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--w16-off", action="store_true", help="infer_w16 = False: split-bf16 planes")
    ap.add_argument("--w16-on", action="store_true", help="infer_w16 = True: the fp16 chain, or an error")
    ap.add_argument("--float", action="store_true", help="an f32 model instead of .half()")
    ap.add_argument("--frames", type=int, nargs="+", default=[1000, 200])
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    cfg = synth.WAVEGLOW_DEFAULT
    m = WaveGlow(**cfg)
    m.load_state_dict(synth.waveglow_state(cfg))
    m = m.cuda().eval()
    if not args.float:
        m.half()
        for c in m.convinv:
            c.float()
    eng = m._eng()
    if hasattr(eng, "infer_w16"):
        eng.infer_w16 = False if args.w16_off else (True if args.w16_on else None)
    os.environ["T2S_F16_GUARD"] = "0"
    out = {"half": not args.float, "channels": cfg["WN_config"]["n_channels"], "lib": os.environ.get("T2S_LIB_PATH", "shipped")}
    gen = torch.Generator().manual_seed(11)
    for frames in args.frames:
        mel = torch.randn(1, cfg["n_mel_channels"], frames, generator=gen).cuda()
        if not args.float:
            mel = mel.half()
        with torch.no_grad():
            audio = m.infer(mel, sigma=0.666)
            torch.cuda.synchronize()
            ts = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                m.infer(mel, sigma=0.666)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
        out["infer_B1_%dframes" % frames] = {"ms": sum(ts) / len(ts), "ms_min": min(ts), "finite": bool(torch.isfinite(audio).all())}
    out["infer_w16"] = bool(getattr(eng, "last_infer_w16", False))
    out["path"] = list(eng.last_path) if eng.last_path is not None else None
    print(json.dumps(out))


if __name__ == "__main__":
    main()
