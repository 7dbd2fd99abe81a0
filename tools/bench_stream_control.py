#!/usr/bin/env python3
"""Control inside the stream on one MI355X (streaming.StreamControl, alignment.AlignmentStream, rate.WarpStream;
the window kernels of csrc/align.hip and csrc/warp.hip).

    python tools/bench_stream_control.py [--runs 12] [--out-dir profiles]

tools/bench_streaming.py's workload: 512 channels, 128 symbols, 1000 frames forced, f32 models, first_frames 32, window_frames 128.
One process, after warm-up runs, the forms alternating (the order swaps from one repetition to the next); the median of --runs
with the spread (max - min).

  stream    synthesize_stream with control=None, with a check whose thresholds never trip, at speed 1.0, at speed 0.8 and with
            timestamps: seconds to the first piece (synchronised behind it) and to the last.  speed 0.8 vocodes 1250 frames, not
            1000: its whole-stream time is not comparable, its first audio is.
  push      one AlignmentStream.push and one WarpStream.push at 64-frame pieces, against the whole-row calls a caller had on the
            prefix: alignment_report(alignments[:, :n]) and warp_mel(mel[:, :, :n]) after every piece.  Per push = a whole pass
            over the pieces, synchronised at its end, divided by their number.
A difference counts only beyond twice the baseline's own spread.  Writes <out>/stream_control.json and <out>/stream_control.md and
prints the JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from text2speech_amd import alignment, rate, streaming  # noqa: E402
from tools.bench_streaming import FRAMES, SEED, SIGMA, models  # noqa: E402

FIRST, WINDOW, PIECE = 32, 128, 64
NEVER = dict(skip_max=10 ** 6, back_max=10 ** 6, stall_max=10 ** 6, end_slack=10 ** 6, min_focus=0.0)
FORMS = (("control=None", None), ("check that never trips", dict(check=True)), ("speed=1.0", dict(speed=1.0)),
         ("speed=0.8", dict(speed=0.8)), ("timestamps=True", dict(timestamps=True)))


def control(kw):
    if kw is None:
        return None
    kw = dict(kw)
    if kw.pop("check", False):
        kw["check"] = alignment.AlignmentCheck(**NEVER)
    return streaming.StreamControl(**kw)


def streamed(taco, wg, ids, kw):
    """(seconds to the first piece, seconds to the last, the control)"""
    ctl = control(kw)
    t0 = time.perf_counter()
    t_first = None
    for _ in streaming.synthesize_stream(taco, wg, ids, seed=SEED, sigma=SIGMA, first_frames=FIRST, window_frames=WINDOW, control=ctl):
        if t_first is None:
            torch.cuda.synchronize()
            t_first = time.perf_counter() - t0
    torch.cuda.synchronize()
    return t_first, time.perf_counter() - t0, ctl


def align_pushes(A, check):
    al = alignment.AlignmentStream(check, A.size(2), A.size(1), A.device)
    edges = list(range(0, A.size(1), PIECE)) + [A.size(1)]
    t0 = time.perf_counter()
    for a, b in zip(edges[:-1], edges[1:]):
        al.push(A[:, a:b], b == A.size(1))
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (len(edges) - 1), al.report()


def align_composed(A, check):
    edges = list(range(0, A.size(1), PIECE)) + [A.size(1)]
    t0 = time.perf_counter()
    for b in edges[1:]:
        rep = alignment.alignment_report(A[:, :b], check=check)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (len(edges) - 1), rep


def warp_pushes(mel, speed):
    ws = rate.WarpStream(mel.size(1), mel.size(2), mel.dtype, mel.device, speed)
    edges = list(range(0, mel.size(2), PIECE)) + [mel.size(2)]
    t0 = time.perf_counter()
    out = [ws.push(mel[:, :, a:b], b == mel.size(2)) for a, b in zip(edges[:-1], edges[1:])]
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (len(edges) - 1), torch.cat(out, 2)


def warp_composed(mel, speed):
    edges = list(range(0, mel.size(2), PIECE)) + [mel.size(2)]
    t0 = time.perf_counter()
    for b in edges[1:]:
        out = rate.warp_mel(mel[:, :, :b], None, speed)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (len(edges) - 1), out.mel


def stats(xs, scale=1e3):
    return dict(median_ms=statistics.median(xs) * scale, min_ms=min(xs) * scale, max_ms=max(xs) * scale, n=len(xs))


def verdict(base, new):
    spread = base["max_ms"] - base["min_ms"]
    d = new["median_ms"] - base["median_ms"]
    if abs(d) <= 2 * spread:
        return "no difference beyond twice the baseline's spread"
    return "%s by %.3f ms (%.2f x)" % ("SLOWER" if d > 0 else "quicker", abs(d), new["median_ms"] / base["median_ms"])


def alternating(runs, a, b):
    ta, tb = [], []
    for r in range(runs):
        for which in ((0, 1) if r % 2 == 0 else (1, 0)):
            (ta if which == 0 else tb).append((a if which == 0 else b)()[0])
    return stats(ta), stats(tb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    ids = (torch.arange(128) % 78 + 2)[None].cuda()
    stderr, sys.stderr = sys.stderr, open(os.devnull, "w")      # the "max decoder steps" warning of every forced 1000-frame run
    try:
        taco, wg = models(False)
        for _, kw in FORMS:                                     # warm-up: the workspaces, the kernels, the page-locked buffers
            for _ in range(2):
                streamed(taco, wg, ids, kw)
        first, total = {n: [] for n, _ in FORMS}, {n: [] for n, _ in FORMS}
        frames = {}
        for r in range(args.runs):
            for name, kw in (FORMS if r % 2 == 0 else FORMS[::-1]):
                a, b, ctl = streamed(taco, wg, ids, kw)
                first[name].append(a)
                total[name].append(b)
                frames[name] = FRAMES if ctl is None else ctl.frames_out
        stream = {n: dict(frames_out=frames[n], first_audio=stats(first[n]), whole_stream=stats(total[n])) for n, _ in FORMS}
        for n, _ in FORMS[1:]:
            for k in ("first_audio", "whole_stream"):
                stream[n][k]["verdict"] = verdict(stream["control=None"][k], stream[n][k])
        out = taco.inference(ids, None, seed=SEED)
        mel, A = out[1].contiguous(), out[3].contiguous()
        check = alignment.AlignmentCheck(max_frames=FRAMES, **NEVER)
        for _ in range(2):
            _, rp = align_pushes(A, check)
            _, rc = align_composed(A, check)
            _, wp = warp_pushes(mel, 0.8)
            _, wc = warp_composed(mel, 0.8)
        same_a = all(torch.equal(x, y) for x, y in zip(rp, rc))
        same_w = torch.equal(wp, wc)
        push = {}
        p, c = alternating(args.runs, lambda: align_pushes(A, check), lambda: align_composed(A, check))
        push["AlignmentStream.push"] = dict(push=p, composed=c, composed_is="alignment_report of the prefix", same_bits=bool(same_a),
                                            verdict=verdict(c, p))
        p, c = alternating(args.runs, lambda: warp_pushes(mel, 0.8), lambda: warp_composed(mel, 0.8))
        push["WarpStream.push"] = dict(push=p, composed=c, composed_is="warp_mel of the prefix at 0.8", same_bits=bool(same_w),
                                       verdict=verdict(c, p))
    finally:
        sys.stderr = stderr
    doc = dict(workload="512 channels, 128 symbols, %d frames forced, f32, first_frames %d, window_frames %d, seed %d; pushes of %d frames"
                        % (FRAMES, FIRST, WINDOW, SEED, PIECE), runs=args.runs, stream=stream, push=push)
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "stream_control.json"), "w") as f:
        json.dump(doc, f, indent=1)
    with open(os.path.join(args.out_dir, "stream_control.md"), "w") as f:
        f.write(markdown(doc))
    print(json.dumps(dict(first_audio_ms={n: stream[n]["first_audio"]["median_ms"] for n in stream},
                          push_ms={n: push[n]["push"]["median_ms"] for n in push})))


def markdown(doc):
    L = ["# Control inside the stream: measured", "",
         "`python tools/bench_stream_control.py` on one MI355X.  %s.  Median of %d, the forms alternating in one process; (min .. max)."
         % (doc["workload"], doc["runs"]), "",
         "| stream | frames vocoded | first audio ms | against control=None | whole stream ms | against control=None |", "|---|---|---|---|---|---|"]
    for n, s in doc["stream"].items():
        f, w = s["first_audio"], s["whole_stream"]
        L.append("| %s | %d | %.2f (%.2f .. %.2f) | %s | %.2f (%.2f .. %.2f) | %s |"
                 % (n, s["frames_out"], f["median_ms"], f["min_ms"], f["max_ms"], f.get("verdict", "-"), w["median_ms"], w["min_ms"],
                    w["max_ms"], w.get("verdict", "-")))
    L += ["", "| per push of %d frames | push ms | the whole-row call on the prefix ms | verdict | the same bits |" % PIECE, "|---|---|---|---|---|"]
    for n, p in doc["push"].items():
        a, b = p["push"], p["composed"]
        L.append("| %s (against %s) | %.3f (%.3f .. %.3f) | %.3f (%.3f .. %.3f) | %s | %s |"
                 % (n, p["composed_is"], a["median_ms"], a["min_ms"], a["max_ms"], b["median_ms"], b["min_ms"], b["max_ms"], p["verdict"],
                    p["same_bits"]))
    return "\n".join(L) + "\n"


if __name__ == "__main__":
    main()
