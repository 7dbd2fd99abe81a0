#!/usr/bin/env python3
"""The true-peak limiter on the device (text2speech_amd/audio.py Limiter, Loudness.normalize_limit_batch, data.py PcmPool.limit,
longform.py limit_long; csrc/limiter.hip) against what a caller has without it: the audio read back, the same limiter in
vectorised numpy / scipy (resample_poly for the envelope, minimum_filter1d for the look-ahead, a convolution for the window),
the result uploaded again.  Synthetic seeded audio; one process, after warm-up calls, the forms alternating (the order swaps from
one repetition to the next), synchronised around each call; median of --reps with the least and the greatest.

  serving   B in {1, 4, 8} float32 rows of 256000 samples at 44800 Hz, brought to -9 LUFS (loud on purpose: the limiter has work) with a ceiling of -1 dB:
              limit      Limiter.limit_batch on rows already at that level (measure: two launches, apply: one)
              norm+limit Loudness.normalize_limit_batch (the loudness measure's four launches, then those three)
              normalize  Loudness.normalize_batch alone (the chain without a limiter)
              host       rows read back, host loudness gain + host limiter per row, float32 copied back
  corpus    --clips int16 clips of 2 to 10 s at 44800 Hz (tools/bench_trim.py's lengths):
              device     pool.limit(limiter) on the pool already in HBM
              host       the host limiter per clip, then PcmPool(limited, 44800): the upload included
              copy       pool.pcm.clone(): one read and one write of the pool
  longform  tools/bench_longform.py's workload through synthesize_long, with and without limit_long(result, limiter, loudness)
A difference counts only beyond twice the baseline's own spread (max - min).  Writes <out>/limiter.json and <out>/limiter.md and
prints the JSON line.  --divide N: N times fewer clips and shorter rows."""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch
from scipy.ndimage import minimum_filter1d
from scipy.signal import resample_poly

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from text2speech_amd import audio as A, data, longform as L  # noqa: E402
from tools.bench_loudness import _time, _verdict, host_gain, noise_rows  # noqa: E402

DEV = "cuda:0"
RATE, TARGET, CEILING_DB = 44800, -9.0, -1.0


def host_limit(u, lim):
    """the limiter of include/t2s_hip.h on one float64 row, vectorised (its sums are scipy's, not the kernel's order)"""
    n, os_, Lk = u.size, lim.oversample, lim.lookahead
    p = np.abs(u)
    if os_ > 1:
        p = np.maximum(p, np.abs(resample_poly(u, os_, 1)).reshape(n, os_).max(axis=1))
    if not (p > lim.ceiling).any():
        return u
    r = np.where(p > lim.ceiling, lim.ceiling / np.maximum(p, 1e-300), 1.0)
    rp = np.concatenate([np.ones(2 * Lk), r, np.ones(2 * Lk)])
    m = minimum_filter1d(rp, 2 * Lk + 1, mode="constant", cval=1.0)[Lk:Lk + n + 2 * Lk]
    s = np.minimum(r, np.convolve(m, A.limiter_window(Lk), mode="valid"))
    return u * s


def serving_case(reps, divide):
    ld, lim = A.Loudness(RATE, TARGET), A.Limiter(RATE, CEILING_DB)
    out = {}
    for name, B, n in (("B1", 1, 256000), ("B4", 4, 256000), ("B8", 8, 256000)):
        n //= divide
        lens_h = [n - 1000 * b for b in range(B)]
        x = torch.from_numpy(noise_rows(B, n, 7 + B)).to(DEV)
        lens = torch.tensor(lens_h, dtype=torch.int32, device=DEV)
        levelled, _ = ld.normalize_batch(x, lens)

        def host():
            a = x.cpu().numpy()
            y = np.zeros_like(a)
            for b, nb in enumerate(lens_h):
                row = a[b, :nb].astype(np.float64)
                y[b, :nb] = host_limit(row * host_gain(row, target=TARGET), lim).astype(np.float32)
            return torch.from_numpy(y).to(DEV)

        got, want = ld.normalize_limit_batch(x, lens, lim)[0], host()
        rel = float(((got - want).double().norm() / want.double().norm()))
        rep = lim.true_peak_batch(x, lens, ld.measure_batch(x, lens).gain)
        st = _time({"limit": (lambda: lim.limit_batch(levelled, lens), 1),
                    "norm+limit": (lambda: ld.normalize_limit_batch(x, lens, lim), 1),
                    "normalize": (lambda: ld.normalize_batch(x, lens), 1), "host": (host, 1)}, reps)
        st.update(rows=B, samples_per_row=n, rel_l2_to_host_form=rel, limited_samples=int(rep.limited.sum()),
                  true_peak_before=float(rep.true_peak.max()), peak_after=float(got.abs().max()),
                  verdict_host=_verdict(st["host"], st["norm+limit"]), verdict_normalize=_verdict(st["normalize"], st["norm+limit"]))
        out[name] = st
    return out


def corpus_case(n_clips, reps, divide):
    gen = np.random.RandomState(1)
    lens = [int(RATE * s) // divide for s in np.linspace(2.0, 10.0, n_clips)]
    gen.shuffle(lens)
    clips = [np.rint(gen.randn(n) * gen.uniform(2000, 12000)).clip(-32768, 32767).astype(np.int16) for n in lens]
    pool = data.PcmPool(clips, RATE, DEV)
    lim = A.Limiter(RATE, CEILING_DB)

    def host():
        out = []
        for c in clips:
            o = host_limit(c.astype(np.float64) / 32768.0, lim)
            out.append(np.rint(32768.0 * o).clip(-32768, 32767).astype(np.int16))
        return data.PcmPool(out, RATE, DEV)

    a, b = pool.limit(lim), host()
    differing = int((a.pcm != b.pcm).sum())
    rep = pool.true_peak(lim)
    st = _time({"device": (lambda: pool.limit(lim), 1), "host": (host, 6), "copy": (lambda: pool.pcm.clone(), 1)}, reps)
    st.update(clips=n_clips, samples=int(pool.pcm.numel()), samples_differing_from_host_form=differing,
              limited_samples=int(rep.limited.sum()), clips_limited=int((rep.limited > 0).sum()),
              largest_code_after=int(a.pcm.to(torch.int32).abs().max()), verdict=_verdict(st["host"], st["device"]),
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
    ld, lim = A.Loudness(L.SAMPLING_RATE, TARGET), A.Limiter(L.SAMPLING_RATE, CEILING_DB)

    def plain():
        return L.synthesize_long(forced, wg, chunks=chunks, seed=BL.SEED, sigma=BL.SIGMA, batch_size=8, denoiser=den,
                                 pause_ms=BL.PAUSE_MS, fade_ms=0)

    def limited():
        return L.limit_long(plain(), lim, ld)

    with contextlib.redirect_stderr(io.StringIO()):             # (the max-decoder-steps warning of every call)
        r = limited()
        rep = lim.true_peak_batch(r.audio, r.length)
        st = _time({"synthesize_long": (plain, 1), "synthesize_long + limit_long": (limited, 1)}, reps)
    st.update(chunks=len(chunks), samples=int(r.length), sample_peak_after=float(rep.sample_peak[0]),
              true_peak_after=float(rep.true_peak[0]), ceiling=lim.ceiling,
              verdict=_verdict(st["synthesize_long"], st["synthesize_long + limit_long"]))
    return st


def _row(name, st):
    return "| %s | %.3f | %.3f | %.3f | %d |" % (name, st["median_ms"], st["min_ms"], st["max_ms"], st["runs"])


def markdown(res):
    head = ["| form | median ms | min | max | runs |", "|---|---|---|---|---|"]
    lines = ["# The true-peak limiter on the device: measured on an MI355X", "",
             "`python tools/bench_limiter.py` (see its docstring for the forms).  Wall-clock ms around a synchronised call, one process,",
             "the forms alternating; median, least and greatest over the stated number of runs.  A difference counts only beyond twice",
             "the baseline's own spread (max - min).", "",
             "## Serving: float32 rows at %d Hz, target %g LUFS, ceiling %g dB" % (RATE, TARGET, CEILING_DB), ""]
    for key, s in res["serving"].items():
        lines += ["### %s: %d rows of %d samples" % (key, s["rows"], s["samples_per_row"]), ""] + head + [
            _row("limit_batch (rows already levelled)", s["limit"]), _row("normalize_limit_batch", s["norm+limit"]),
            _row("normalize_batch alone", s["normalize"]), _row("host: read back, numpy / scipy, copy back", s["host"]), "",
            "Against the host form: %s.  Against `normalize_batch` alone (the baseline; \"device\" is `normalize_limit_batch`): %s."
            % (s["verdict_host"], s["verdict_normalize"]),
            "%d samples over the ceiling, true peak before %.3f, largest sample after %.6f; rel-L2 to the host form %.2e." % (
                s["limited_samples"], s["true_peak_before"], s["peak_after"], s["rel_l2_to_host_form"]), ""]
    c = res["corpus"]
    lines += ["## Corpus: %d int16 clips of 2 to 10 s, %d samples" % (c["clips"], c["samples"]), ""] + head + [
        _row("pool.limit (pool in HBM)", c["device"]), _row("host: numpy / scipy per clip + upload", c["host"]),
        _row("pool.pcm.clone()", c["copy"]), "",
        "%s.  %.1f times the copy of the pool.  %d clips limited, %d samples over the ceiling, largest code after %d.  Samples that"
        % (c["verdict"], c["device_over_copy"], c["clips_limited"], c["limited_samples"], c["largest_code_after"]),
        "differ from the host form: %d (its sums run in another order; a last-bit difference moves a sample that lies on a"
        % c["samples_differing_from_host_form"], "half-integer).", ""]
    f = res["longform"]
    lines += ["## Long form: %d chunks, %d samples" % (f["chunks"], f["samples"]), ""] + head + [
        _row("synthesize_long", f["synthesize_long"]), _row("synthesize_long + limit_long(loudness=)", f["synthesize_long + limit_long"]), "",
        "%s (here \"device\" is the chain with limit_long, the baseline the chain without).  The limited utterance: sample peak %.6f,"
        % (f["verdict"], f["sample_peak_after"]), "true peak %.6f, ceiling %.6f." % (f["true_peak_after"], f["ceiling"]), ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--clips", type=int, default=600)
    ap.add_argument("--divide", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X: a time taken elsewhere says nothing"
    res = {"reps": args.reps, "torch_threads": torch.get_num_threads()}
    for name, case in (("serving", lambda: serving_case(args.reps, args.divide)),
                       ("corpus", lambda: corpus_case(max(2, args.clips // args.divide), args.reps, args.divide)),
                       ("longform", lambda: longform_case(args.reps, args.divide))):
        res[name] = case()
        print("[bench_limiter] %s done" % name, file=sys.stderr, flush=True)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "limiter.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    with open(os.path.join(args.out, "limiter.md"), "w") as f:
        f.write(markdown(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
