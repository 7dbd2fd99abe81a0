#!/usr/bin/env python3
"""Sample-rate conversion on the device (text2speech_amd/audio.py Resampler, data.py PcmPool.resample; csrc/resample.hip) against
what a caller has without it: scipy.signal.resample_poly on the host.  Synthetic seeded audio; in one process, after warm-up calls, the
forms alternating (the order swaps from one repetition to the next), synchronised around each call.

  ingest    a corpus of --clips int16 clips of 2 to 10 s at 44100 Hz brought to 44800 Hz (64 / 63, 1281 taps, 21 per output):
              device    PcmPool(clips, 44100) - one upload - then .resample(44800)
              resample  .resample(44800) alone on the pool already in HBM; its bytes/s count every input sample read once and every
                        output sample written once (2 bytes each), against the 6.29 TB/s a copy kernel reaches on this chip
              host      resample_poly of every clip in float64, rint, saturate to int16, then PcmPool(converted, 44800)
            the two pools must be equal sample for sample, which is checked before anything is timed
  serving   B in {1, 4, 8} rows of 256000 samples (1000 frames) from WaveGlow.infer_batch at 44800 Hz, to 48000 (15 / 14) and to 16000
            (5 / 14), config.json-default WaveGlow with synthetic weights:
              resample_batch   Resampler.resample_batch on denoise_batch's two results
              host             the same rows read back, resample_poly in float64 per row, float32 copied back
              denoise_batch, infer_batch on the same batch: what share of a served batch the conversion is
Writes <out>/resample.json and <out>/resample.md and prints the JSON line.  --divide N: N times fewer clips and shorter rows."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from text2speech_amd import data, synth  # noqa: E402
from text2speech_amd.audio import Denoiser, Resampler  # noqa: E402
from text2speech_amd.glow import WaveGlow  # noqa: E402

DEV = "cuda:0"
HBM_COPY_BYTES_PER_S = 6.29e12          # measured float4 copy on an MI355X


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


def _host_int16(clip, up, down):
    from scipy.signal import resample_poly
    y = np.rint(resample_poly(clip.astype(np.float64), up, down))
    return np.clip(y, -32768, 32767).astype(np.int16)


def ingest_case(n_clips, reps, divide):
    src, dst = 44100, 44800
    gen = np.random.RandomState(1)
    lens = [int(src * s) // divide for s in np.linspace(2.0, 10.0, n_clips)]
    gen.shuffle(lens)
    clips = [gen.randint(-20000, 20000, n).astype(np.int16) for n in lens]
    rs = Resampler(src, dst, device=DEV)
    pool = data.PcmPool(clips, src, DEV)

    def device():
        return data.PcmPool(clips, src, DEV).resample(dst)

    def host():
        return data.PcmPool([_host_int16(c, rs.up, rs.down) for c in clips], dst, DEV)

    a, b = device(), host()
    differing = int((a.pcm != b.pcm).sum())
    assert a.lengths.tolist() == b.lengths.tolist(), "the two forms differ in length"
    st = _time({"device": (device, 1), "resample": (lambda: pool.resample(dst), 1), "host": (host, 4)}, reps)
    n_in, n_out = int(pool.pcm.numel()), int(a.pcm.numel())
    taps = -(-rs.n_taps // rs.up)
    sec = st["resample"]["median_ms"] * 1e-3
    st.update(clips=n_clips, samples_in=n_in, samples_out=n_out, ratio="%d/%d" % (rs.up, rs.down), n_taps=rs.n_taps,
              dfma_per_output=taps, samples_differing_from_host_form=differing,
              host_over_device=round(st["host"]["median_ms"] / st["device"]["median_ms"], 1),
              resample_bytes_per_s=round(2 * (n_in + n_out) / sec, 0),
              resample_share_of_hbm_copy_rate=round(2 * (n_in + n_out) / sec / HBM_COPY_BYTES_PER_S, 4),
              resample_dfma_per_s=round(n_out * taps / sec, 0))
    return st


def serving_case(reps, divide):
    from scipy.signal import resample_poly
    cfg = synth.WAVEGLOW_DEFAULT
    m = WaveGlow(**cfg)
    m.load_state_dict(synth.waveglow_state(cfg))
    m = m.to(DEV).eval()
    dn = Denoiser(m).to(DEV)
    gen = torch.Generator().manual_seed(17)
    frames_all = [max(3, f // divide) for f in (1000, 930, 860, 750, 670, 580, 470, 375)]
    out = {"frames": frames_all, "samples_per_row": 256 * frames_all[0]}
    for B in (1, 4, 8):
        frames = frames_all[:B]
        mel = torch.randn(B, 80, max(frames), generator=gen).to(DEV)
        lens = torch.tensor(frames)
        with torch.no_grad():
            audio, alen = m.infer_batch(mel, lens, sigma=0.666)
            den, dlen = dn.denoise_batch(audio, alen, 0.1)
        n_host = [256 * f for f in frames]
        case = {}
        for rate in (48000, 16000):
            rs = Resampler(44800, rate, device=DEV)

            def host():
                x = den[:, 0].cpu().numpy()
                rows = [resample_poly(x[b, :n].astype(np.float64), rs.up, rs.down).astype(np.float32) for b, n in enumerate(n_host)]
                y = np.zeros((B, rs.out_length(x.shape[1])), dtype=np.float32)
                for b, r in enumerate(rows):
                    y[b, :r.size] = r
                return torch.from_numpy(y).to(DEV)

            got, _ = rs.resample_batch(den, dlen)
            worst = float((got[:, 0] - host()).abs().max())
            st = _time({"resample_batch": (lambda: rs.resample_batch(den, dlen), 1), "host": (host, 1)}, reps)
            taps = -(-rs.n_taps // rs.up)
            n_in, n_out = sum(n_host), sum(rs.out_length(n) for n in n_host)
            sec = st["resample_batch"]["median_ms"] * 1e-3
            st.update(ratio="%d/%d" % (rs.up, rs.down), n_taps=rs.n_taps, dfma_per_output=taps, worst_abs_difference_from_host_form=worst,
                      host_over_device=round(st["host"]["median_ms"] / st["resample_batch"]["median_ms"], 1),
                      bytes_per_s=round(4 * (n_in + n_out) / sec, 0),
                      share_of_hbm_copy_rate=round(4 * (n_in + n_out) / sec / HBM_COPY_BYTES_PER_S, 4),
                      dfma_per_s=round(n_out * taps / sec, 0))
            case["to_%d" % rate] = st
        with torch.no_grad():
            rest = _time({"denoise_batch": (lambda: dn.denoise_batch(audio, alen, 0.1), 1),
                          "infer_batch": (lambda: m.infer_batch(mel, lens, sigma=0.666), 1)}, max(3, reps // 2))
        case.update(rest)
        served = rest["denoise_batch"]["median_ms"] + rest["infer_batch"]["median_ms"]
        for rate in (48000, 16000):
            r = case["to_%d" % rate]["resample_batch"]["median_ms"]
            case["to_%d" % rate]["share_of_served_batch"] = round(r / (served + r), 5)
        out["B%d" % B] = case
    return out


def _row(name, st):
    return "| %s | %.3f | %.3f | %.3f | %d |" % (name, st["median_ms"], st["min_ms"], st["max_ms"], st["runs"])


def markdown(res):
    ing, srv = res["ingest"], res["serving"]
    lines = ["# Sample-rate conversion on the device: measured on an MI355X", "",
             "`python tools/bench_resample.py` (see its docstring for the forms).  Wall-clock ms around a synchronised call, one process, the",
             "forms alternating; median, least and greatest over the stated number of runs.", "",
             "## Ingest: %d clips of 2 to 10 s, 44100 -> 44800 Hz (%s, %d taps, %d DFMA per output)" % (
                 ing["clips"], ing["ratio"], ing["n_taps"], ing["dfma_per_output"]), "",
             "%d samples in, %d out.  Samples that differ between the device pool and the host form: %d." % (
                 ing["samples_in"], ing["samples_out"], ing["samples_differing_from_host_form"]), "",
             "| form | median ms | min | max | runs |", "|---|---|---|---|---|",
             _row("device: upload + PcmPool.resample", ing["device"]), _row("PcmPool.resample alone (pool in HBM)", ing["resample"]),
             _row("host: scipy resample_poly per clip + upload", ing["host"]), "",
             "host / device: %.1f.  PcmPool.resample alone moves %.3g bytes/s of input read once and output written once, %.2f %% of the"
             % (ing["host_over_device"], ing["resample_bytes_per_s"], 100 * ing["resample_share_of_hbm_copy_rate"]),
             "6.29 TB/s copy rate, at %.3g DFMA/s.  HBM does not bound it; which of the per-tap costs (the LDS read of the filter, the L1 read of"
             % ing["resample_dfma_per_s"],
             "the sample, the DFMA itself) does has not been measured - no counter run was made.",
             "", "## Serving: rows of %d samples at 44800 Hz (frames %s)" % (srv["samples_per_row"], srv["frames"]), ""]
    for key in [k for k in srv if k.startswith("B")]:
        c = srv[key]
        lines += ["### %s" % key, "", "| call | median ms | min | max | runs |", "|---|---|---|---|---|"]
        for rate in (48000, 16000):
            t = c["to_%d" % rate]
            lines += [_row("resample_batch -> %d (%s, %d DFMA per output)" % (rate, t["ratio"], t["dfma_per_output"]), t["resample_batch"]),
                      _row("host: read back, resample_poly, copy back -> %d" % rate, t["host"])]
        lines += [_row("denoise_batch", c["denoise_batch"]), _row("infer_batch", c["infer_batch"]), ""]
        for rate in (48000, 16000):
            t = c["to_%d" % rate]
            lines.append("-> %d: host / device %.1f; %.3g bytes/s (%.2f %% of the copy rate), %.3g DFMA/s; %.3f %% of the served batch; worst "
                         "|device - host form| %.2e." % (rate, t["host_over_device"], t["bytes_per_s"], 100 * t["share_of_hbm_copy_rate"],
                                                          t["dfma_per_s"], 100 * t["share_of_served_batch"],
                                                          t["worst_abs_difference_from_host_form"]))
        lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--clips", type=int, default=600)
    ap.add_argument("--divide", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X: a time taken elsewhere says nothing"
    res = {"reps": args.reps, "torch_threads": torch.get_num_threads(),
           "ingest": ingest_case(max(2, args.clips // args.divide), args.reps, args.divide), "serving": serving_case(args.reps, args.divide)}
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "resample.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    with open(os.path.join(args.out, "resample.md"), "w") as f:
        f.write(markdown(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
