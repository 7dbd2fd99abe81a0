#!/usr/bin/env python3
"""BS.1770 loudness normalisation on the device (text2speech_amd/audio.py Loudness, data.py PcmPool.normalize_loudness,
longform.py normalize_long; csrc/loudness.hip) against what a caller has without it: the audio read back, scipy.signal.lfilter for
the K-weighting, numpy for blocks and gates, the scaled audio uploaded again.  Synthetic seeded audio; one process, after warm-up
calls, the forms alternating (the order swaps from one repetition to the next), synchronised around each call; median of --reps
with the least and the greatest.

  serving   B in {1, 4, 8} float32 rows of 256000 samples at 44800 Hz, and one joined row of 1290000 samples:
              device   Loudness.normalize_batch (measure: four launches, apply: one)
              measure  Loudness.measure_batch alone
              host     rows read back, lfilter + numpy gating per row, float32 copied back
  corpus    --clips int16 clips of 2 to 10 s at 44800 Hz (tools/bench_trim.py's lengths):
              device   pool.normalize_loudness(-23) on the pool already in HBM
              host     the same steps per clip in numpy, then PcmPool(levelled, 44800): the upload included
              copy     pool.pcm.clone(): one read and one write of the pool
  longform  tools/bench_longform.py's workload through synthesize_long, with and without normalize_long behind it
A difference counts only beyond twice the baseline's own spread (max - min).  Writes <out>/loudness.json and <out>/loudness.md and
prints the JSON line.  --divide N: N times fewer clips and shorter rows."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
from scipy.signal import lfilter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from text2speech_amd import audio as A, data, longform as L  # noqa: E402

DEV = "cuda:0"
RATE, TARGET = 44800, -23.0


def _once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _stats(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "runs": len(ms)}


def _time(runs, reps):
    """runs: name -> (fn, every): fn is timed in every `every`-th repetition (a slow host form need not run as often)"""
    for fn, _ in runs.values():
        fn()
    ms = {k: [] for k in runs}
    order = list(runs)
    for r in range(reps):
        for k in (order if r % 2 == 0 else order[::-1]):
            if r % runs[k][1] == 0:
                ms[k].append(_once(runs[k][0]))
    return {k: _stats(v) for k, v in ms.items()}


def _verdict(base, dev):
    """quicker / slower / no difference: beyond twice the baseline's own spread"""
    spread = base["max_ms"] - base["min_ms"]
    d = base["median_ms"] - dev["median_ms"]
    return "no difference beyond twice the baseline's spread" if abs(d) <= 2 * spread else (
        "device quicker, %.1f x" % (base["median_ms"] / dev["median_ms"]) if d > 0 else
        "device SLOWER, %.1f x" % (dev["median_ms"] / base["median_ms"]))


# ---- the host form --------------------------------------------------------------------------------------------------------------------
def host_gain(x64, fs=RATE, target=TARGET, peak_limit=None):
    """the gain of one row (float64 samples in the units the measure counts), vectorised numpy"""
    (b1, a1), (b2, a2) = A.loudness_coefficients(fs)
    h = A.loudness_hop(fs)
    nh = x64.size // h
    if nh < 4:
        return 1.0
    y = lfilter(b2, a2, lfilter(b1, a1, x64))[:nh * h]
    z = np.square(y).reshape(nh, h).sum(axis=1)
    ms_j = (z[:-3] + z[1:-2] + z[2:-1] + z[3:]) / (4.0 * h)
    keep = ms_j[ms_j > A.LOUD_GATE_ABS]
    if keep.size == 0:
        return 1.0
    keep = keep[keep > 0.1 * keep.mean()]
    g = float(np.sqrt(10.0 ** ((target + 0.691) / 10.0) / keep.mean()))
    if peak_limit is not None:
        peak = float(np.abs(x64).max())
        if peak * g > peak_limit:
            g = peak_limit / peak
    return g


def noise_rows(B, n, seed):
    gen = np.random.default_rng(seed)
    level = np.repeat(gen.choice([0.2, 0.02, 0.1, 0.3], size=n // 20000 + 1), 20000)[:n]
    return (gen.standard_normal((B, n)) * level).clip(-1, 1).astype(np.float32)


def serving_case(reps, divide):
    ld = A.Loudness(RATE, TARGET)
    out = {}
    for name, B, n in (("B1", 1, 256000), ("B4", 4, 256000), ("B8", 8, 256000), ("joined", 1, 1290000)):
        n //= divide
        lens_h = [n - 1000 * b for b in range(B)]
        x = torch.from_numpy(noise_rows(B, n, 7 + B)).to(DEV)
        lens = torch.tensor(lens_h, dtype=torch.int32, device=DEV)

        def host():
            a = x.cpu().numpy()
            y = np.zeros_like(a)
            for b, nb in enumerate(lens_h):
                row = a[b, :nb].astype(np.float64)
                y[b, :nb] = (row * host_gain(row)).astype(np.float32)
            return torch.from_numpy(y).to(DEV)

        got, want = ld.normalize_batch(x, lens)[0], host()
        rel = float(((got - want).double().norm() / want.double().norm()))
        st = _time({"device": (lambda: ld.normalize_batch(x, lens), 1), "measure": (lambda: ld.measure_batch(x, lens), 1),
                    "host": (host, 1)}, reps)
        st.update(rows=B, samples_per_row=n, rel_l2_to_host_form=rel, verdict=_verdict(st["host"], st["device"]),
                  bytes_per_s=round(4 * 3 * sum(lens_h) / (st["device"]["median_ms"] * 1e-3), 0))
        out[name] = st
    return out


def corpus_case(n_clips, reps, divide):
    gen = np.random.RandomState(1)
    lens = [int(RATE * s) // divide for s in np.linspace(2.0, 10.0, n_clips)]
    gen.shuffle(lens)
    clips = [np.rint(gen.randn(n) * gen.uniform(300, 6000)).clip(-32768, 32767).astype(np.int16) for n in lens]
    pool = data.PcmPool(clips, RATE, DEV)
    limit = 32767 / 32768

    def host():
        lev = []
        for c in clips:
            g = host_gain(c.astype(np.float64) / 32768.0, peak_limit=limit)
            lev.append(np.rint(c.astype(np.float64) * g).clip(-32768, 32767).astype(np.int16))
        return data.PcmPool(lev, RATE, DEV)

    a, b = pool.normalize_loudness(TARGET, allow_unmeasured=True), host()
    differing = int((a.pcm != b.pcm).sum())
    st = _time({"device": (lambda: pool.normalize_loudness(TARGET, allow_unmeasured=True), 1), "host": (host, 4),
                "copy": (lambda: pool.pcm.clone(), 1)}, reps)
    st.update(clips=n_clips, samples=int(pool.pcm.numel()), samples_differing_from_host_form=differing,
              verdict=_verdict(st["host"], st["device"]),
              device_over_copy=round(st["device"]["median_ms"] / st["copy"]["median_ms"], 1))
    return st


def longform_case(reps, divide):
    from tools import bench_longform as BL
    from text2speech_amd import synth
    from text2speech_amd.glow import WaveGlow
    from text2speech_amd.tacotron import Tacotron
    taco = Tacotron(synth.TACOTRON_HPARAMS, 80, num_speakers=2)
    taco.load_state_dict(synth.tacotron_state())
    taco = taco.to(DEV).eval()
    wg = WaveGlow(**synth.WAVEGLOW_DEFAULT)
    wg.load_state_dict(synth.waveglow_state())
    wg = wg.to(DEV).eval()
    den = A.Denoiser(wg)
    chunks = BL.make_chunks(max(2, 16 // divide))
    counts = [L.n_symbols(c) for c in chunks]
    frames_of = {k: max(3, round((150 + (k - 40) * 250 / 88) / divide)) for k in counts}
    forced = BL.Forced(taco, frames_of)
    ld = A.Loudness(L.SAMPLING_RATE, TARGET, peak_limit=0.99)

    def plain():
        return L.synthesize_long(forced, wg, chunks=chunks, seed=BL.SEED, sigma=BL.SIGMA, batch_size=8, denoiser=den,
                                 pause_ms=BL.PAUSE_MS, fade_ms=0)

    def levelled():
        return L.normalize_long(plain(), ld)

    with contextlib.redirect_stderr(io.StringIO()):             # (the max-decoder-steps warning of every call)
        r = levelled()
        rep = ld.measure_batch(r.audio, r.length)
        st = _time({"synthesize_long": (plain, 1), "synthesize_long + normalize_long": (levelled, 1)}, reps)
    st.update(chunks=len(chunks), samples=int(r.length), lufs_after=float(rep.lufs[0]), flags_after=int(rep.flags[0]),
              verdict=_verdict(st["synthesize_long"], st["synthesize_long + normalize_long"]))
    return st


def _row(name, st):
    return "| %s | %.3f | %.3f | %.3f | %d |" % (name, st["median_ms"], st["min_ms"], st["max_ms"], st["runs"])


def markdown(res):
    head = ["| form | median ms | min | max | runs |", "|---|---|---|---|---|"]
    lines = ["# Loudness normalisation on the device: measured on an MI355X", "",
             "`python tools/bench_loudness.py` (see its docstring for the forms).  Wall-clock ms around a synchronised call, one process,",
             "the forms alternating; median, least and greatest over the stated number of runs.  A difference counts only beyond twice",
             "the baseline's own spread (max - min).", "", "## Serving: float32 rows at %d Hz, target %g LUFS" % (RATE, TARGET), ""]
    for key, s in res["serving"].items():
        lines += ["### %s: %d rows of %d samples" % (key, s["rows"], s["samples_per_row"]), ""] + head + [
            _row("normalize_batch (measure + apply)", s["device"]), _row("measure_batch alone", s["measure"]),
            _row("host: read back, lfilter + numpy, copy back", s["host"]), "",
            "%s.  %.3g bytes/s (two reads and one write of every sample, 4 bytes each); rel-L2 to the host form %.2e." % (
                s["verdict"], s["bytes_per_s"], s["rel_l2_to_host_form"]), ""]
    c = res["corpus"]
    lines += ["## Corpus: %d int16 clips of 2 to 10 s, %d samples" % (c["clips"], c["samples"]), ""] + head + [
        _row("pool.normalize_loudness (pool in HBM)", c["device"]), _row("host: numpy per clip + upload", c["host"]),
        _row("pool.pcm.clone()", c["copy"]), "",
        "%s.  %.1f times the copy of the pool.  Samples that differ from the host form: %d (a last-bit difference of the gain moves a"
        % (c["verdict"], c["device_over_copy"], c["samples_differing_from_host_form"]),
        "sample that lies on a half-integer).", ""]
    f = res["longform"]
    lines += ["## Long form: %d chunks, %d samples" % (f["chunks"], f["samples"]), ""] + head + [
        _row("synthesize_long", f["synthesize_long"]), _row("synthesize_long + normalize_long", f["synthesize_long + normalize_long"]), "",
        "%s (here \"device\" is the chain with normalize_long, the baseline the chain without).  The levelled utterance measures"
        % f["verdict"], "%.4f LUFS, flags %d." % (f["lufs_after"], f["flags_after"]), ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--clips", type=int, default=600)
    ap.add_argument("--divide", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X: a time taken elsewhere says nothing"
    res = {"reps": args.reps, "torch_threads": torch.get_num_threads(), "serving": serving_case(args.reps, args.divide),
           "corpus": corpus_case(max(2, args.clips // args.divide), args.reps, args.divide),
           "longform": longform_case(args.reps, args.divide)}
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "loudness.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    with open(os.path.join(args.out, "loudness.md"), "w") as f:
        f.write(markdown(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
