#!/usr/bin/env python3
"""IIR filtering in HBM on one MI355X (audio.SosFilter / FilterStream, PcmPool.filter, DeliveryStream(pre_filter=, post_filter=);
csrc/sosfilt.hip).

    python tools/bench_filter.py [--runs 12] [--out-dir profiles] [--skip-stream] [--bench-steps K --parent-lib PATH]

One process, after warm-up runs, the forms alternating (the order swaps from one repetition to the next); the median of --runs with
(min .. max).  A difference counts only beyond twice the larger spread.

  batch     SosFilter.filter_batch of B rows of 256 000 samples, B = 1 / 4 / 8, 1 and 4 sections, against what a caller had: read
            the rows back, scipy.signal.sosfilt in float64, upload the float32 result.
  pool      PcmPool.filter of 600 int16 clips of 2 - 10 s at 22 050 Hz (an 80 Hz high-pass, 2 sections) against the host form - read
            back, sosfilt every clip, round, upload - and the number of samples in which the two differ.
  push      the pieces of one plain synthesize_stream run pushed through a DeliveryStream to 8 kHz mu-law, without filters and with
            de-emphasis in front of the resampler and the telephone band behind it; per push.
  stream    first audio and whole-stream time of synthesize_stream(delivery=) with those two streams
            (tools/bench_streaming.py's workload: 512 channels, 128 symbols, 1000 frames forced).
  bench     with --bench-steps: bench.py --gpus 1's headline in child processes, this tree's library and (with --parent-lib, a
            library built from the parent commit) the parent's, alternating.
Writes <out>/filter.json and <out>/filter.md and prints the JSON line."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch
from scipy.signal import sosfilt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from text2speech_amd import audio as A, data  # noqa: E402
from tools.bench_delivery import stats, streamed  # noqa: E402

SRC, GAIN = 44800, 2.0


def verdict(base, new):
    spread = max(base["max_ms"] - base["min_ms"], new["max_ms"] - new["min_ms"])
    d = new["median_ms"] - base["median_ms"]
    if abs(d) <= 2 * spread:
        return "no difference beyond twice the larger spread"
    return "%s by %.3f ms (%.2f x)" % ("SLOWER" if d > 0 else "quicker", abs(d), new["median_ms"] / base["median_ms"])


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def alternate(forms, runs):
    """forms: name -> callable; -> name -> seconds per run, the order swapping from one repetition to the next"""
    names = list(forms)
    for n in names:
        for _ in range(2):
            forms[n]()
    out = {n: [] for n in names}
    for r in range(runs):
        for n in (names if r % 2 == 0 else names[::-1]):
            out[n].append(timed(forms[n])[0])
    return out


def bench_batch(runs):
    res = {}
    for sections, sos in ((1, A.sos_deemphasis(0.97)), (4, A.sos_butter(4, (300.0, 3400.0), "bandpass", 8000))):
        f = A.SosFilter(sos)
        for B in (1, 4, 8):
            x = (0.3 * torch.randn(B, 256000, generator=torch.Generator().manual_seed(B))).cuda()

            def host():
                return torch.from_numpy(sosfilt(sos, x.cpu().numpy().astype(np.float64), axis=-1).astype(np.float32)).cuda()
            t = alternate({"device": lambda: f.filter_batch(x)[0], "host": host}, runs)
            d, h = stats(t["device"]), stats(t["host"])
            err = float((f.filter_batch(x)[0].double() - host().double()).abs().max())
            res["%d section%s, B = %d" % (sections, "s" if sections > 1 else "", B)] = dict(
                device=d, host=h, verdict=verdict(h, d), max_abs_difference=err)
    return res


def bench_pool(runs):
    fs = 22050
    rng = np.random.RandomState(1)
    clips = [np.clip(np.rint(4000.0 * rng.randn(int(n))), -32768, 32767).astype(np.int16) for n in rng.randint(2 * fs, 10 * fs + 1, 600)]
    pool = data.PcmPool(clips, fs)
    sos = A.sos_butter(4, 80.0, "highpass", fs)
    f = A.SosFilter(sos, fs)
    offs, lens = pool.offsets.tolist(), pool.lengths.tolist()

    def host():
        pcm = pool.pcm.cpu().numpy()
        out = np.empty_like(pcm)
        for o, n in zip(offs, lens):
            out[o:o + n] = np.clip(np.rint(sosfilt(sos, pcm[o:o + n].astype(np.float64))), -32768, 32767).astype(np.int16)
        return torch.from_numpy(out).cuda()
    t = alternate({"device": lambda: pool.filter(f).pcm, "host": host}, runs)
    d, h = stats(t["device"]), stats(t["host"])
    differing = int((pool.filter(f).pcm != host()).sum())
    return dict(clips=len(clips), samples=int(pool.pcm.numel()), device=d, host=h, verdict=verdict(h, d), differing_samples=differing)


def _streams(limiter):
    pre = A.SosFilter(A.sos_deemphasis(0.97), SRC)
    post = A.SosFilter(A.sos_butter(4, (300.0, 3400.0), "bandpass", 8000), 8000)
    return {"without filters": lambda: A.DeliveryStream(SRC, 8000, limiter=limiter, gain=GAIN, encoding="ulaw"),
            "de-emphasis + telephone band": lambda: A.DeliveryStream(SRC, 8000, limiter=limiter, gain=GAIN, encoding="ulaw", pre_filter=pre,
                                                                     post_filter=post)}


def bench_stream(runs):
    from tools.bench_streaming import models
    ids = (torch.arange(128) % 78 + 2)[None].cuda()
    stderr, sys.stderr = sys.stderr, open(os.devnull, "w")      # the "max decoder steps" warning of every forced 1000-frame run
    try:
        taco, wg = models(False)
        makers = _streams(A.Limiter(8000))
        for _ in range(2):
            _, _, plain = streamed(taco, wg, ids, None)
        for m in makers.values():
            for _ in range(2):
                streamed(taco, wg, ids, m)
        names = list(makers)
        first, total = {n: [] for n in names}, {n: [] for n in names}
        for r in range(runs):
            for n in (names if r % 2 == 0 else names[::-1]):
                a, b, _ = streamed(taco, wg, ids, makers[n])
                first[n].append(a)
                total[n].append(b)

        def pushes(make):
            ds = make().open(1)
            return [ds.push(p, q == len(plain) - 1) for q, p in enumerate(plain)]
        t = alternate({n: (lambda m=m: pushes(m)) for n, m in makers.items()}, runs)
    finally:
        sys.stderr = stderr
    stream = {n: dict(first_audio=stats(first[n]), whole_stream=stats(total[n])) for n in names}
    push = {n: stats([v / len(plain) for v in t[n]]) for n in names}
    for k in ("first_audio", "whole_stream"):
        stream[names[1]][k]["verdict"] = verdict(stream[names[0]][k], stream[names[1]][k])
    push[names[1]]["verdict"] = verdict(push[names[0]], push[names[1]])
    return dict(pieces=len(plain), stream=stream, push=push)


def bench_headline(steps, parent_lib, runs):
    """bench.py's line in child processes; with parent_lib the two libraries alternate"""
    def one(lib):
        env = dict(os.environ)
        if lib:
            env["T2S_LIB_PATH"] = lib
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "3",
                              "--no-cpu-baseline", "--no-tacotron", "--no-train"], env=env, capture_output=True, text=True, timeout=600)
        line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
        return json.loads(line)
    forms = [("this tree", None)] + ([("parent", parent_lib)] if parent_lib else [])
    res = {n: [] for n, _ in forms}
    for r in range(runs):
        for n, lib in (forms if r % 2 == 0 else forms[::-1]):
            res[n].append(one(lib))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--skip-stream", action="store_true")
    ap.add_argument("--bench-steps", type=int, default=0)
    ap.add_argument("--bench-runs", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    args = ap.parse_args()
    doc = dict(runs=args.runs, batch=bench_batch(args.runs), pool=bench_pool(args.runs))
    if not args.skip_stream:
        doc["delivery"] = bench_stream(args.runs)
    if args.bench_steps:
        doc["bench"] = bench_headline(args.bench_steps, args.parent_lib, args.bench_runs)
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "filter.json"), "w") as f:
        json.dump(doc, f, indent=1)
    with open(os.path.join(args.out_dir, "filter.md"), "w") as f:
        f.write(markdown(doc))
    print(json.dumps(dict(batch_ms={k: v["device"]["median_ms"] for k, v in doc["batch"].items()},
                          pool_ms=doc["pool"]["device"]["median_ms"], pool_host_ms=doc["pool"]["host"]["median_ms"])))


def _cell(s):
    return "%.3f (%.3f .. %.3f)" % (s["median_ms"], s["min_ms"], s["max_ms"])


def markdown(doc):
    L = ["# IIR filtering in HBM: measured", "",
         "`python tools/bench_filter.py` on one MI355X.  Median of %d, the forms alternating in one process; (min .. max).  A difference"
         % doc["runs"], "counts only beyond twice the larger spread.", "",
         "| filter_batch, rows of 256 000 | device ms | read back + sosfilt + upload ms | verdict | max abs difference |", "|---|---|---|---|---|"]
    for n, b in doc["batch"].items():
        L.append("| %s | %s | %s | %s | %.2e |" % (n, _cell(b["device"]), _cell(b["host"]), b["verdict"], b["max_abs_difference"]))
    p = doc["pool"]
    L += ["", "| pool: %d int16 clips, %d samples, 80 Hz high-pass | device ms | host form ms | verdict | differing samples |" % (p["clips"], p["samples"]),
          "|---|---|---|---|---|", "| PcmPool.filter | %s | %s | %s | %d |" % (_cell(p["device"]), _cell(p["host"]), p["verdict"], p["differing_samples"])]
    if "delivery" in doc:
        d = doc["delivery"]
        L += ["", "| DeliveryStream to 8 kHz mu-law, %d pieces | per push ms | first audio ms | whole stream ms |" % d["pieces"], "|---|---|---|---|"]
        for n in d["push"]:
            s = d["stream"][n]
            L.append("| %s | %s | %s | %s |" % (n, _cell(d["push"][n]), _cell(s["first_audio"]), _cell(s["whole_stream"])))
        n = list(d["push"])[1]
        L += ["", "With filters against without: per push %s; first audio %s; whole stream %s."
              % (d["push"][n]["verdict"], d["stream"][n]["first_audio"]["verdict"], d["stream"][n]["whole_stream"]["verdict"])]
    else:
        L += ["", "The DeliveryStream and synthesize_stream legs were skipped in this run (`--skip-stream`): not measured."]
    if "bench" in doc:
        L += ["", "`bench.py --gpus 1` in child processes:", ""]
        for n, lines in doc["bench"].items():
            L.append("* %s: %s" % (n, "; ".join(json.dumps(ln) for ln in lines)))
    else:
        L += ["", "`bench.py`'s headline against the parent commit was not taken by this run."]
    return "\n".join(L) + "\n"


if __name__ == "__main__":
    main()
