#!/usr/bin/env python3
"""Delivery inside the stream on one MI355X (audio.DeliveryStream, synthesize_stream(delivery=); csrc/delivery.hip).

    python tools/bench_delivery.py [--runs 12] [--out-dir profiles]

tools/bench_streaming.py's workload: 512 channels, 128 symbols, 1000 frames forced, f32 models, first_frames 32, window_frames 128.
One process, after warm-up runs, the forms alternating (the order swaps from one repetition to the next); the median of --runs
with the spread (max - min).

  stream    synthesize_stream plain, with delivery to 8 kHz mu-law and with delivery to 48 kHz int16 (a limiter at -1 dB and a gain
            of 2 in both): seconds to the first piece (synchronised behind it) and to the last.
  push      the pieces of one plain run pushed through a DeliveryStream, against the same stream composed from the calls that
            existed before: torch.cat of a tail and the piece, Resampler.forward, Limiter.limit_batch, a slice, to_pcm16 (the tail
            long enough for both filters).  Per push = a whole pass over the pieces, synchronised at its end, divided by their number.
A difference counts only beyond twice the baseline's own spread.  Writes <out>/delivery.json and <out>/delivery.md and prints the
JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from text2speech_amd import audio as A, streaming  # noqa: E402
from tools.bench_streaming import SEED, SIGMA, models  # noqa: E402

SRC, FIRST, WINDOW, GAIN = 44800, 32, 128, 2.0
FORMS = (("plain", None, None), ("8 kHz mu-law", 8000, "ulaw"), ("48 kHz int16", 48000, "pcm16"))


def delivery(rate, encoding, limiters):
    return A.DeliveryStream(SRC, rate, limiter=limiters[rate], gain=GAIN, encoding=encoding)


def streamed(taco, wg, ids, make):
    """(seconds to the first piece, seconds to the last, pieces)"""
    t0 = time.perf_counter()
    t_first, pieces = None, []
    for a in streaming.synthesize_stream(taco, wg, ids, seed=SEED, sigma=SIGMA, first_frames=FIRST, window_frames=WINDOW,
                                         delivery=make):
        if t_first is None:
            torch.cuda.synchronize()
            t_first = time.perf_counter() - t0
        pieces.append(a)
    torch.cuda.synchronize()
    return t_first, time.perf_counter() - t0, pieces


def pushes(pieces, rate, encoding, limiters):
    ds = delivery(rate, encoding, limiters).open(1)
    t0 = time.perf_counter()
    outs = [ds.push(p, q == len(pieces) - 1) for q, p in enumerate(pieces)]
    torch.cuda.synchronize()
    return time.perf_counter() - t0, outs


def composed(pieces, rate, encoding, limiters, rs):
    """what a caller had: keep a tail of the source, compute the tail and the piece again, keep the new samples"""
    lim = limiters[rate]
    tail_n = -(-rs.n_taps // rs.up) + -(-2 * lim.reach * rs.down // rs.up) + 1
    gain = torch.full((1,), GAIN, dtype=torch.float64, device="cuda")
    enc = A.to_pcm16 if encoding == "pcm16" else A.to_ulaw
    tail, seen, given, outs = None, 0, 0, []
    t0 = time.perf_counter()
    for q, p in enumerate(pieces):
        x = p if tail is None else torch.cat([tail, p], 1)
        seen += p.size(1)
        y = lim.limit_batch(rs.forward(x), gain=gain)[0]
        total = rs.out_length(seen)
        upto = total if q == len(pieces) - 1 else max(given, total - lim.reach - -(-(rs.n_taps // 2) // rs.down))
        if upto > given:
            outs.append(enc(y[:, y.size(1) - (total - given):y.size(1) - (total - upto)]))
        given = upto
        tail = x[:, -tail_n:]
    torch.cuda.synchronize()
    return time.perf_counter() - t0, outs


def stats(xs, scale=1e3):
    return dict(median_ms=statistics.median(xs) * scale, min_ms=min(xs) * scale, max_ms=max(xs) * scale, n=len(xs))


def verdict(base, new):
    spread = base["max_ms"] - base["min_ms"]
    d = new["median_ms"] - base["median_ms"]
    if abs(d) <= 2 * spread:
        return "no difference beyond twice the baseline's spread"
    return "%s by %.3f ms (%.2f x)" % ("SLOWER" if d > 0 else "quicker", abs(d), new["median_ms"] / base["median_ms"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    ids = (torch.arange(128) % 78 + 2)[None].cuda()
    stderr, sys.stderr = sys.stderr, open(os.devnull, "w")      # the "max decoder steps" warning of every forced 1000-frame run
    try:
        taco, wg = models(False)
        limiters = {r: A.Limiter(r) for r in (8000, 48000)}
        makers = {name: (None if rate is None else (lambda rate=rate, enc=enc: delivery(rate, enc, limiters))) for name, rate, enc in FORMS}
        plain = None
        for name in makers:                                     # warm-up: the workspaces, the kernels, the tables
            for _ in range(2):
                _, _, got = streamed(taco, wg, ids, makers[name])
            if name == "plain":
                plain = got
        first, total = {n: [] for n in makers}, {n: [] for n in makers}
        order = list(makers)
        for r in range(args.runs):
            for name in (order if r % 2 == 0 else order[::-1]):
                a, b, _ = streamed(taco, wg, ids, makers[name])
                first[name].append(a)
                total[name].append(b)
        stream = {n: dict(first_audio=stats(first[n]), whole_stream=stats(total[n])) for n in makers}
        for n in order[1:]:
            for k in ("first_audio", "whole_stream"):
                stream[n][k]["verdict"] = verdict(stream["plain"][k], stream[n][k])
        push = {}
        for name, rate, enc in FORMS[1:]:
            rs = A.Resampler(SRC, rate)
            for _ in range(2):
                _, a = pushes(plain, rate, enc, limiters)
                _, b = composed(plain, rate, enc, limiters, rs)
            same = torch.equal(torch.cat(a, 1), torch.cat(b, 1))
            tp, tc = [], []
            for r in range(args.runs):
                for which in ((0, 1) if r % 2 == 0 else (1, 0)):
                    if which == 0:
                        tp.append(pushes(plain, rate, enc, limiters)[0] / len(plain))
                    else:
                        tc.append(composed(plain, rate, enc, limiters, rs)[0] / len(plain))
            push[name] = dict(pieces=len(plain), samples_in=[int(p.size(1)) for p in plain], push=stats(tp), composed=stats(tc),
                              composed_gives_the_same_bits=bool(same))
            push[name]["verdict"] = verdict(push[name]["composed"], push[name]["push"])
    finally:
        sys.stderr = stderr
    doc = dict(workload="512 channels, 128 symbols, 1000 frames forced, f32, first_frames %d, window_frames %d, seed %d; gain %.1f, "
                        "ceiling -1 dB" % (FIRST, WINDOW, SEED, GAIN), runs=args.runs, stream=stream, push=push)
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "delivery.json"), "w") as f:
        json.dump(doc, f, indent=1)
    with open(os.path.join(args.out_dir, "delivery.md"), "w") as f:
        f.write(markdown(doc))
    print(json.dumps(dict(first_audio_ms={n: stream[n]["first_audio"]["median_ms"] for n in stream},
                          push_ms={n: push[n]["push"]["median_ms"] for n in push})))


def markdown(doc):
    L = ["# Delivery inside the stream: measured", "",
         "`python tools/bench_delivery.py` on one MI355X.  %s.  Median of %d, the forms alternating in one process; (min .. max)."
         % (doc["workload"], doc["runs"]), "",
         "| stream | first audio ms | against plain | whole stream ms | against plain |", "|---|---|---|---|---|"]
    for n, s in doc["stream"].items():
        f, w = s["first_audio"], s["whole_stream"]
        L.append("| %s | %.2f (%.2f .. %.2f) | %s | %.2f (%.2f .. %.2f) | %s |"
                 % (n, f["median_ms"], f["min_ms"], f["max_ms"], f.get("verdict", "-"), w["median_ms"], w["min_ms"], w["max_ms"],
                    w.get("verdict", "-")))
    L += ["", "| per push, %d pieces | DeliveryStream.push ms | composed from existing calls ms | verdict | composed gives the same bits |"
          % next(iter(doc["push"].values()))["pieces"], "|---|---|---|---|---|"]
    for n, p in doc["push"].items():
        a, b = p["push"], p["composed"]
        L.append("| %s | %.3f (%.3f .. %.3f) | %.3f (%.3f .. %.3f) | %s | %s |"
                 % (n, a["median_ms"], a["min_ms"], a["max_ms"], b["median_ms"], b["min_ms"], b["max_ms"], p["verdict"],
                    p["composed_gives_the_same_bits"]))
    return "\n".join(L) + "\n"


if __name__ == "__main__":
    main()
