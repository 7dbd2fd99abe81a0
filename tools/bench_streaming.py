#!/usr/bin/env python3
"""Streaming synthesis on one MI355X: time to the first audio piece, total time and the worst (window compute time / audio time it
delivers), beside the whole-utterance chain measured in the same process, alternating; and the halo curve.

    python tools/bench_streaming.py [--runs 12] [--out-dir profiles]

The workload is tools/bench_e2e.py's: 512 channels, 128 symbols, 1000 frames forced (gate threshold 2, max_decoder_steps 1000), as
f32 models and as .half() ones.  For every first_frames in {16, 32, 64} x window_frames in {64, 128, 256}: `runs` pairs of
(streamed, whole) runs, the median of each and its spread (max - min over the runs).  A streamed run synchronises after its first
piece and after its last, nowhere else; the per-window ratios come from one more run that synchronises after every piece.
Writes streaming.json and streaming.md into --out-dir and prints one JSON summary line."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from text2speech_amd import streaming, synth  # noqa: E402
from text2speech_amd.glow import WaveGlow  # noqa: E402
from text2speech_amd.tacotron import Tacotron  # noqa: E402

SEED, SIGMA, FRAMES, RATE = 1234, 0.666, 1000, 22050.0


def models(half, **wg_state):
    taco = Tacotron(dict(synth.TACOTRON_HPARAMS), 80, num_speakers=2)
    taco.load_state_dict(synth.tacotron_state())
    taco = taco.cuda().eval()
    cfg = synth.WAVEGLOW_DEFAULT
    wg = WaveGlow(**cfg)
    wg.load_state_dict(synth.waveglow_state(cfg, **wg_state))
    wg = WaveGlow.remove_weightnorm(wg).cuda().eval()
    if half:
        taco.half()
        wg.half()
        for c in wg.convinv:
            c.float()
    taco.decoder.gate_threshold, taco.decoder.max_decoder_steps = 2.0, FRAMES
    return taco, wg


def whole(taco, wg, ids):
    t0 = time.perf_counter()
    out = taco.inference(ids, None, seed=SEED)
    audio = wg.infer(out[1], sigma=SIGMA, seed=SEED)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, audio


def streamed(taco, wg, ids, first, window, every_piece=False):
    """(seconds to the first piece, total seconds, [(seconds since the piece before, samples)] with every_piece, pieces)"""
    t0 = time.perf_counter()
    t_first, t_prev, per, pieces = None, t0, [], []
    for a in streaming.synthesize_stream(taco, wg, ids, seed=SEED, sigma=SIGMA, first_frames=first, window_frames=window):
        if t_first is None or every_piece:
            torch.cuda.synchronize()
            now = time.perf_counter()
            if t_first is None:
                t_first = now - t0
            per.append((now - t_prev, int(a.size(1))))
            t_prev = now
        pieces.append(a)
    torch.cuda.synchronize()
    return t_first, time.perf_counter() - t0, per, pieces


def med_spread(xs):
    return statistics.median(xs) * 1e3, (max(xs) - min(xs)) * 1e3


def halo_curve(half=False):
    """rel-L2 against infer(seed=) of the middle window [136, 264) of a 400-frame mel at shrinking halos, default and stress weights"""
    rows = []
    mel = torch.randn(1, 80, 400, generator=torch.Generator().manual_seed(5)).cuda()
    for label, kw in (("default", {}), ("stress (end_std 0.03, wn_gain 1.25)", dict(end_std=0.03, wn_gain=1.25))):
        _, wg = models(half, **kw)
        ref = wg.infer(mel, sigma=SIGMA, seed=SEED)[:, 256 * 136:256 * 264].double()
        for halo in ((99, 96), (48, 48), (32, 32), (24, 24), (16, 16)):
            got = wg.infer_window(mel, 136, 264, sigma=SIGMA, seed=SEED, halo=halo).double()
            rows.append(dict(weights=label, halo=list(halo), rel_l2=float((got - ref).norm() / ref.norm()),
                             bit_equal=bool(torch.equal(got, ref))))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    ids = (torch.arange(128) % 78 + 2)[None].cuda()
    stderr, sys.stderr = sys.stderr, open(os.devnull, "w")      # the "max decoder steps" warning of every forced 1000-frame run
    results = []
    try:
        for half in (False, True):
            taco, wg = models(half)
            for _ in range(2):
                _, ref = whole(taco, wg, ids)
            for first in (16, 32, 64):
                for window in (64, 128, 256):
                    _, _, _, pieces = streamed(taco, wg, ids, first, window)        # warm-up: the stream's workspaces
                    got = torch.cat(pieces, 1)
                    rel = float((got.double() - ref.double()).norm() / ref.double().norm())
                    tf, tt, tw = [], [], []
                    for _ in range(args.runs):
                        a, b, _, _ = streamed(taco, wg, ids, first, window)
                        tf.append(a)
                        tt.append(b)
                        tw.append(whole(taco, wg, ids)[0])
                    _, _, per, _ = streamed(taco, wg, ids, first, window, every_piece=True)
                    ratios = [dt / (n / RATE) for dt, n in per]
                    r = dict(dtype="half" if half else "f32", first_frames=first, window_frames=window, pieces=len(pieces),
                             samples=int(got.size(1)), rel_l2_vs_whole=rel, bit_equal=bool(torch.equal(got, ref)),
                             worst_window_compute_over_audio=max(ratios[1:]) if len(ratios) > 1 else None,
                             first_piece_compute_over_audio=ratios[0])
                    for name, xs in (("first_audio_ms", tf), ("stream_total_ms", tt), ("whole_chain_ms", tw)):
                        r[name], r[name + "_spread"] = med_spread(xs)
                    results.append(r)
        curve = halo_curve()
    finally:
        sys.stderr = stderr
    os.makedirs(args.out_dir, exist_ok=True)
    doc = dict(workload="512 channels, 128 symbols, %d frames forced, seed %d, sigma %.3f" % (FRAMES, SEED, SIGMA), runs=args.runs,
               halo=list(streaming.vocoder_halo(synth.WAVEGLOW_DEFAULT)), results=results, halo_curve=curve)
    with open(os.path.join(args.out_dir, "streaming.json"), "w") as f:
        json.dump(doc, f, indent=1)
    with open(os.path.join(args.out_dir, "streaming.md"), "w") as f:
        f.write(markdown(doc))
    best = min((r for r in results if r["dtype"] == "f32"), key=lambda r: r["first_audio_ms"])
    print(json.dumps(dict(first_audio_ms=best["first_audio_ms"], whole_chain_ms=best["whole_chain_ms"],
                          first_frames=best["first_frames"], window_frames=best["window_frames"])))


def markdown(doc):
    L = ["# Streaming synthesis: time to the first audio", "",
         "`python tools/bench_streaming.py` on one MI355X.  %s; the median of %d runs, streamed and whole-utterance runs alternating in one"
         % (doc["workload"], doc["runs"]),
         "process; spread = max - min over those runs.  Exact halo %s frames.  `worst window` is the largest (compute time of a window"
         % (tuple(doc["halo"]),),
         "behind the first / audio time it delivers) of a run that synchronises after every piece: below 1 the stream keeps ahead of",
         "playback.", "",
         "| dtype | first | window | pieces | first audio ms (spread) | stream total ms (spread) | whole chain ms (spread) | worst window | vs whole rel-L2 | bit-equal |",
         "|---|---|---|---|---|---|---|---|---|---|"]
    for r in doc["results"]:
        L.append("| %s | %d | %d | %d | %.2f (%.2f) | %.2f (%.2f) | %.2f (%.2f) | %s | %.1e | %s |"
                 % (r["dtype"], r["first_frames"], r["window_frames"], r["pieces"], r["first_audio_ms"], r["first_audio_ms_spread"],
                    r["stream_total_ms"], r["stream_total_ms_spread"], r["whole_chain_ms"], r["whole_chain_ms_spread"],
                    "-" if r["worst_window_compute_over_audio"] is None else "%.3f" % r["worst_window_compute_over_audio"],
                    r["rel_l2_vs_whole"], r["bit_equal"]))
    L += ["", "## The halo curve", "",
          "rel-L2 against `infer(seed=)` of the middle window [136, 264) of a 400-frame random mel, 512 channels, f32, as the halo shrinks.",
          "These are synthetic weights; trained checkpoints are unmeasured, and their influence may decay more slowly.", "",
          "| weights | halo (left, right) | rel-L2 | bit-equal |", "|---|---|---|---|"]
    for c in doc["halo_curve"]:
        L.append("| %s | (%d, %d) | %.2e | %s |" % (c["weights"], c["halo"][0], c["halo"][1], c["rel_l2"], c["bit_equal"]))
    return "\n".join(L) + "\n"


if __name__ == "__main__":
    main()
