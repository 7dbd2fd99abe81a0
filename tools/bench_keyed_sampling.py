#!/usr/bin/env python3
"""Keyed sampling (text2speech_amd/sampling.py, csrc/sampling.hip) against the default draws: what a seed costs or saves per call.
config.json-default WaveGlow (512 channels) with synthetic weights, sigma 0.666, in one process, after warm-up calls, the forms
alternating (the order swaps from one repetition to the next), synchronised around each call; median ms over --reps runs.

  solo      B = 1 at 200 and 1000 frames:  infer()  against  infer(seed=)
  batch     B = 8 on the 400 ... 150-frame series:  infer_batch()  against  infer_batch(seeds=)
  kernel    t2s_wg_noise_keyed alone on the [B, n_group, L] buffer of each case above, beside torch.randn + multiply + slice-assign
            as the default path fills the same buffer
  masks     t2s_bernoulli_mask_keyed alone at [1000, 8, 512] beside t2s_bernoulli_mask over the same bytes

--unseeded-only: the unseeded rows alone - what a library without the keyed entry points can run (T2S_LIB_PATH=<the parent commit's
build> for the A/B against the parent: the rows must agree, since no existing kernel is compiled differently).  Writes
<out>/keyed_sampling<tag>.json and prints the JSON line; --md also writes <out>/keyed_sampling.md from this run."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from text2speech_amd import _lib, synth  # noqa: E402
from text2speech_amd.glow import WaveGlow  # noqa: E402

DEV = "cuda:0"
SIGMA = 0.666
BATCH_FRAMES = (400, 365, 330, 295, 260, 220, 185, 150)


def _once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "runs": len(ms)}


def _time(runs, reps):
    for fn in runs.values():
        fn()
        fn()
    ms = {k: [] for k in runs}
    order = list(runs)
    for r in range(reps):
        for k in (order if r % 2 == 0 else order[::-1]):
            ms[k].append(_once(runs[k]))
    return {k: _stats(v) for k, v in ms.items()}


def _model():
    cfg = synth.WAVEGLOW_DEFAULT
    m = WaveGlow(**cfg)
    m.load_state_dict(synth.waveglow_state(cfg))
    return m.to(DEV).eval()


def _fill_default(m, z, sigma):
    """the default path's fill of z, statement for statement (glow.py _infer)"""
    B, G, L = z.shape
    nf = torch.randn(B, m.n_remaining_channels, L, dtype=torch.float32, device=DEV)
    ne = [torch.randn(B, m.n_early_size, L, dtype=torch.float32, device=DEV) for _ in m._eng().early_flows()]
    z[:, G - m.n_remaining_channels:] = sigma * nf
    off = G - m.n_remaining_channels
    for t in ne:
        z[:, off - m.n_early_size:off] = sigma * t
        off -= m.n_early_size


def run(reps, divide, unseeded_only):
    m = _model()
    gen = torch.Generator().manual_seed(23)
    G = m.n_group
    res = {}
    cases = [("solo_%d" % f, (max(3, f // divide),)) for f in (200, 1000)] + [("batch_8", tuple(max(3, f // divide) for f in BATCH_FRAMES))]
    for name, frames in cases:
        B, F_ = len(frames), max(frames)
        mel = torch.randn(B, 80, F_, generator=gen).to(DEV)
        seeds = torch.arange(1, B + 1, dtype=torch.int64, device=DEV)
        L = F_ * 256 // G
        z = torch.empty(B, G, L, dtype=torch.float32, device=DEV)
        with torch.no_grad():
            if B == 1:
                runs = {"unseeded": lambda: m.infer(mel, sigma=SIGMA)}
                if not unseeded_only:
                    runs["seeded"] = lambda: m.infer(mel, sigma=SIGMA, seed=1)
            else:
                lens = torch.tensor(frames)
                runs = {"unseeded": lambda: m.infer_batch(mel, lens, sigma=SIGMA)}
                if not unseeded_only:
                    runs["seeded"] = lambda: m.infer_batch(mel, lens, sigma=SIGMA, seeds=seeds)
            runs["fill_default"] = lambda: _fill_default(m, z, SIGMA)
            if not unseeded_only:
                runs["fill_keyed"] = lambda: _lib.call("t2s_wg_noise_keyed", _lib.ptr(z), B, G, L, _lib.ptr(seeds), SIGMA, None,
                                                       _lib.current_stream())
            st = _time(runs, reps)
        st.update(frames=list(frames), z_elements=B * G * L)
        if not unseeded_only:
            st["seeded_minus_unseeded_ms"] = round(st["seeded"]["median_ms"] - st["unseeded"]["median_ms"], 4)
            st["keyed_bytes_per_s"] = round(4 * B * G * L / (st["fill_keyed"]["median_ms"] * 1e-3), 0)
        res[name] = st
    n, B, row = max(2, 1000 // divide), 8, 512
    mk = torch.empty(n, B, row, dtype=torch.uint8, device=DEV)
    seeds = torch.arange(1, B + 1, dtype=torch.int64, device=DEV)
    runs = {"flat": lambda: _lib.call("t2s_bernoulli_mask", _lib.ptr(mk), mk.numel(), 1, 0, 0.5, _lib.current_stream())}
    if not unseeded_only:
        runs["keyed"] = lambda: _lib.call("t2s_bernoulli_mask_keyed", _lib.ptr(mk), n, B, row, _lib.ptr(seeds), 0.5, _lib.current_stream())
    res["masks"] = dict(_time(runs, reps), shape=[n, B, row])
    return res


def markdown(res):
    head = ["| form | median ms | min | max | runs |", "|---|---|---|---|---|"]
    row = lambda name, st: "| %s | %.3f | %.3f | %.3f | %d |" % (name, st["median_ms"], st["min_ms"], st["max_ms"], st["runs"])
    lines = ["# Keyed sampling: measured on an MI355X", "",
             "`python tools/bench_keyed_sampling.py --md` (see its docstring for the forms).  Wall-clock ms around a synchronised call, one",
             "process, the forms alternating; median, least and greatest over the stated number of runs.  config.json-default WaveGlow,",
             "512 channels, synthetic weights, sigma %.3f, library %s." % (SIGMA, res["library"]), ""]
    for key, title in (("solo_200", "infer, B = 1"), ("solo_1000", "infer, B = 1"), ("batch_8", "infer_batch, B = 8")):
        s = res[key]
        lines += ["## %s, frames %s (z: %d floats)" % (title, s["frames"], s["z_elements"]), ""] + head
        lines += [row("without a seed", s["unseeded"])]
        if "seeded" in s:
            lines += [row("with seed(s)", s["seeded"])]
        lines += [row("the default fill alone: torch.randn, multiply, slice-assign", s["fill_default"])]
        if "fill_keyed" in s:
            lines += [row("t2s_wg_noise_keyed alone", s["fill_keyed"]), "",
                      "seeded - unseeded: %+.3f ms; the keyed kernel writes %.3g bytes/s." % (s["seeded_minus_unseeded_ms"], s["keyed_bytes_per_s"])]
        lines += [""]
    s = res["masks"]
    lines += ["## prenet masks %s" % s["shape"], ""] + head + [row("t2s_bernoulli_mask over the whole buffer", s["flat"])]
    if "keyed" in s:
        lines += [row("t2s_bernoulli_mask_keyed", s["keyed"])]
    return "\n".join(lines + [""])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--divide", type=int, default=1)
    ap.add_argument("--unseeded-only", action="store_true")
    ap.add_argument("--tag", default="")
    ap.add_argument("--md", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X: a time taken elsewhere says nothing"
    res = {"reps": args.reps, "library": os.path.relpath(_lib.LIB_PATH, ROOT), "unseeded_only": args.unseeded_only}
    res.update(run(args.reps, args.divide, args.unseeded_only))
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "keyed_sampling%s.json" % args.tag), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    if args.md:
        with open(os.path.join(args.out, "keyed_sampling.md"), "w") as f:
            f.write(markdown(res))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
