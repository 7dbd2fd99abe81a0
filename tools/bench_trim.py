#!/usr/bin/env python3
"""Peak rescaling and silence trimming on the device (text2speech_amd/audio.py Trimmer, data.py PcmPool.rescale_trim; csrc/trim.hip)
against what a caller has without it: a vectorised numpy implementation of the same steps on the host.  librosa is not a dependency
of this project, so the host baseline is the restatement of its formulas (tests/trim_ref.py states them), written for speed: one
pass of squares per clip, hop-block sums combined into frames.  Synthetic seeded audio; in one process, after warm-up calls, the
forms alternating (the order swaps from one repetition to the next), synchronised around each call.

  corpus    --clips int16 clips of 2 to 10 s at 44800 Hz (the lengths of tools/bench_resample.py's pool), each a loud stretch between
            a quiet lead and tail, through rescale_trim(0.999, 23) at (512, 128), reflect padding:
              device      PcmPool(clips, 44800) - one upload - then .rescale_trim(0.999, 23)
              trim        .rescale_trim(0.999, 23) alone on the pool already in HBM
              host        the numpy form per clip, then PcmPool(trimmed, 44800)
              copy        pool.pcm.clone(): one read and one write of the pool, the traffic floor
              energy / bounds / gather   the three launches of rescale_trim one by one on prepared tables; the energy pass's bytes/s
                          count every sample read once (2 bytes), beside the 6.29 TB/s a copy kernel reaches on this chip
            the two pools must be equal sample for sample, which is checked before anything is timed
  serving   B in {1, 4, 8} rows of 256000 samples (1000 frames) from WaveGlow.infer_batch and Denoiser.denoise_batch, the last tenth of
            every entry made quiet, config.json-default WaveGlow with synthetic weights:
              trim_batch   Trimmer(rescaling_max=0.999).trim_batch on denoise_batch's two results
              host         the same rows read back, the numpy form per row, float32 copied back
              denoise_batch, infer_batch on the same batch: what share of a served batch the trim is
Writes <out>/trim.json and <out>/trim.md and prints the JSON line.  --divide N: N times fewer clips and shorter rows."""
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
from text2speech_amd import _lib, data, synth  # noqa: E402
from text2speech_amd.audio import Denoiser, Trimmer, _to_device  # noqa: E402
from text2speech_amd.glow import WaveGlow  # noqa: E402

DEV = "cuda:0"
HBM_COPY_BYTES_PER_S = 6.29e12          # measured float4 copy on an MI355X
FL, HOP, TOP_DB, RESCALE = 512, 128, 23.0, 0.999


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


# ---- the host form ----------------------------------------------------------------------------------------------------------------------
def host_bounds(x, unit_gain, rescaling_max=RESCALE, top_db=TOP_DB, fl=FL, hop=HOP):
    """(start, end, peak) of one clip: reflect padding, frame energies from hop-block sums (hop divides fl), the log-free rule"""
    n, pad, k = x.size, fl // 2, fl // hop
    xp = np.pad(x.astype(np.float64), pad, mode="reflect")
    nf = 1 + (n + 2 * pad - fl) // hop
    blocks = np.square(xp[:(nf + k - 1) * hop]).reshape(nf + k - 1, hop).sum(axis=1)
    E = blocks[:nf].copy()
    for j in range(1, k):
        E += blocks[j:j + nf]
    peak = float(np.abs(x).max()) if x.dtype != np.int16 else float(np.abs(x.astype(np.int32)).max())
    e_max = float(E.max())
    if not e_max > 0 or not np.isfinite(e_max):
        return 0, 0, peak
    g = rescaling_max / peak if rescaling_max is not None and peak > 0 else unit_gain
    F = 1e-10 * fl / (g * g)
    loud = np.flatnonzero(np.maximum(E, F) > 10.0 ** (-top_db / 10.0) * max(e_max, F))
    return int(loud[0]) * hop, min(n, (int(loud[-1]) + 1) * hop), peak


def host_int16(x):
    s, e, peak = host_bounds(x, 1.0 / 32768.0)
    y = np.rint(x[s:e].astype(np.float64) * ((RESCALE * 32768.0) / peak))
    return np.clip(y, -32768, 32767).astype(np.int16)


def host_float(x):
    s, e, peak = host_bounds(x, 1.0)
    return (x[s:e].astype(np.float64) * (RESCALE / peak)).astype(np.float32)


# ---- the corpus -------------------------------------------------------------------------------------------------------------------------
def corpus_clips(n_clips, divide):
    gen = np.random.RandomState(1)
    lens = [int(44800 * s) // divide for s in np.linspace(2.0, 10.0, n_clips)]
    gen.shuffle(lens)
    clips = []
    for n in lens:
        lead, tail = int(n * gen.uniform(0.03, 0.12)), int(n * gen.uniform(0.03, 0.12))
        env = np.full(n, 30.0 / 20000.0)
        m = n - lead - tail
        t = np.arange(m)
        env[lead:lead + m] = np.minimum(1.0, np.minimum(t + 1, m - t) / 2000.0)
        clips.append(np.rint(gen.randint(-20000, 20000, n) * env).astype(np.int16))
    return clips


def corpus_case(n_clips, reps, divide):
    clips = corpus_clips(n_clips, divide)
    pool = data.PcmPool(clips, 44800, DEV)

    def device():
        return data.PcmPool(clips, 44800, DEV).rescale_trim(RESCALE, TOP_DB)

    def host():
        return data.PcmPool([host_int16(c) for c in clips], 44800, DEV)

    a, b = device(), host()
    assert a.lengths.tolist() == b.lengths.tolist(), "the two forms differ in length"
    differing = int((a.pcm != b.pcm).sum())

    # the three launches one by one, on tables prepared as rescale_trim prepares them
    tr = Trimmer(FL, HOP, TOP_DB, "reflect", RESCALE)
    n = len(pool)
    frames = 1 + pool.lengths // HOP
    table3 = _to_device(torch.stack([pool.offsets, pool.lengths, torch.cumsum(frames, 0) - frames], 1).contiguous(), DEV)
    table4 = _to_device(torch.stack([pool.offsets, pool.lengths, a.offsets, a.lengths], 1).contiguous(), DEV)
    energy = torch.empty(int(frames.sum()), dtype=torch.float64, device=DEV)
    stats = torch.empty(n, 2, dtype=torch.float64, device=DEV)
    bounds = torch.empty(n, 2, dtype=torch.int64, device=DEV)
    dst = torch.empty_like(a.pcm)
    p, st_ = _lib.ptr, _lib.current_stream
    shape = (FL, HOP, 0, int(frames.max()))

    def energy_pass():
        _lib.call("t2s_trim_energy", p(pool.pcm), 0, pool.pcm.numel(), p(table3), n, *shape, p(energy), energy.numel(), p(stats), st_())

    def bounds_pass():
        _lib.call("t2s_trim_bounds", p(table3), n, 0, pool.pcm.numel(), *shape, p(energy), energy.numel(), p(stats), TOP_DB, 1, RESCALE,
                  0.0, p(bounds), st_())

    def gather_pass():
        _lib.call("t2s_trim_gather", p(pool.pcm), 0, pool.pcm.numel(), p(table4), n, p(bounds), p(stats), RESCALE, 0.0, p(dst), 0,
                  dst.numel(), int(a.lengths.max()), None, st_())

    energy_pass(), bounds_pass(), gather_pass()
    torch.cuda.synchronize()
    assert torch.equal(dst, a.pcm), "the launches one by one differ from rescale_trim"
    st = _time({"device": (device, 1), "trim": (lambda: pool.rescale_trim(RESCALE, TOP_DB), 1), "host": (host, 4),
                "copy": (lambda: pool.pcm.clone(), 1), "energy": (energy_pass, 1), "bounds": (bounds_pass, 1), "gather": (gather_pass, 1)},
               reps)
    n_in, n_out = int(pool.pcm.numel()), int(a.pcm.numel())
    sec = st["energy"]["median_ms"] * 1e-3
    st.update(clips=n_clips, samples_in=n_in, samples_out=n_out, frames=int(frames.sum()), samples_differing_from_host_form=differing,
              host_over_device=round(st["host"]["median_ms"] / st["device"]["median_ms"], 1),
              trim_over_copy=round(st["trim"]["median_ms"] / st["copy"]["median_ms"], 1),
              energy_bytes_per_s=round(2 * n_in / sec, 0),
              energy_share_of_hbm_copy_rate=round(2 * n_in / sec / HBM_COPY_BYTES_PER_S, 4),
              one_read_of_the_pool_ms=round(2 * n_in / HBM_COPY_BYTES_PER_S * 1e3, 4),
              gather_bytes_per_s=round(2 * (2 * n_out) / (st["gather"]["median_ms"] * 1e-3), 0))
    return st


# ---- serving ------------------------------------------------------------------------------------------------------------------------------
def serving_case(reps, divide):
    cfg = synth.WAVEGLOW_DEFAULT
    m = WaveGlow(**cfg)
    m.load_state_dict(synth.waveglow_state(cfg))
    m = m.to(DEV).eval()
    dn = Denoiser(m).to(DEV)
    tr = Trimmer(FL, HOP, TOP_DB, "reflect", RESCALE)
    gen = torch.Generator().manual_seed(17)
    frames_all = [max(3, f // divide) for f in (1000, 930, 860, 750, 670, 580, 470, 375)]
    out = {"frames": frames_all, "samples_per_row": 256 * frames_all[0]}
    for B in (1, 4, 8):
        frames = frames_all[:B]
        mel = torch.randn(B, 80, max(frames), generator=gen).to(DEV)
        lens = torch.tensor(frames)
        with torch.no_grad():
            audio, alen = m.infer_batch(mel, lens, sigma=0.666)
            for b, f in enumerate(frames):
                audio[b, 256 * f - 256 * f // 10:256 * f] *= 1e-4
            den, dlen = dn.denoise_batch(audio, alen, 0.1)
        n_host = [256 * f for f in frames]

        def host():
            x = den[:, 0].cpu().numpy()
            y = np.zeros_like(x)
            kept = []
            for b, n_b in enumerate(n_host):
                r = host_float(x[b, :n_b])
                y[b, :r.size] = r
                kept.append(r.size)
            return torch.from_numpy(y).to(DEV), kept

        got, got_len = tr.trim_batch(den, dlen)
        want, kept = host()
        st = _time({"trim_batch": (lambda: tr.trim_batch(den, dlen), 1), "host": (host, 1)}, reps)
        with torch.no_grad():
            rest = _time({"denoise_batch": (lambda: dn.denoise_batch(audio, alen, 0.1), 1),
                          "infer_batch": (lambda: m.infer_batch(mel, lens, sigma=0.666), 1)}, max(3, reps // 2))
        st.update(rest)
        served = rest["denoise_batch"]["median_ms"] + rest["infer_batch"]["median_ms"]
        t = st["trim_batch"]["median_ms"]
        st.update(kept=kept, lengths_equal_host_form=got_len.tolist() == kept,
                  values_differing_from_host_form=int((got[:, 0] != want).sum()),
                  host_over_device=round(st["host"]["median_ms"] / t, 1), share_of_served_batch=round(t / (served + t), 5),
                  bytes_per_s=round(4 * (sum(n_host) + sum(kept)) / (t * 1e-3), 0))
        out["B%d" % B] = st
    return out


def _row(name, st):
    return "| %s | %.3f | %.3f | %.3f | %d |" % (name, st["median_ms"], st["min_ms"], st["max_ms"], st["runs"])


def markdown(res):
    c, srv = res["corpus"], res["serving"]
    head = ["| form | median ms | min | max | runs |", "|---|---|---|---|---|"]
    lines = ["# Peak rescaling and silence trimming on the device: measured on an MI355X", "",
             "`python tools/bench_trim.py` (see its docstring for the forms).  Wall-clock ms around a synchronised call, one process, the",
             "forms alternating; median, least and greatest over the stated number of runs.  The host baseline is a vectorised numpy",
             "restatement of librosa's formulas (librosa is not a dependency of this project), not librosa itself.", "",
             "## Corpus: %d clips of 2 to 10 s at 44800 Hz, rescale_trim(%g, %g), frames (%d, %d)" % (c["clips"], RESCALE, TOP_DB, FL, HOP), "",
             "%d samples in, %d kept, %d frames.  Samples that differ between the device pool and the host form: %d." % (
                 c["samples_in"], c["samples_out"], c["frames"], c["samples_differing_from_host_form"]), ""] + head + [
             _row("device: upload + PcmPool.rescale_trim", c["device"]), _row("PcmPool.rescale_trim alone (pool in HBM)", c["trim"]),
             _row("host: numpy per clip + upload", c["host"]), _row("pool.pcm.clone(): the traffic floor", c["copy"]),
             _row("energy pass alone", c["energy"]), _row("bounds pass alone", c["bounds"]), _row("gather alone", c["gather"]), "",
             "host / device: %.1f.  rescale_trim alone takes %.1f times the copy of the pool; it also reads the cut points back and uploads"
             % (c["host_over_device"], c["trim_over_copy"]),
             "two tables, which the three launches one by one do not.  The energy pass reads %.3g bytes/s of samples, each counted once,"
             % c["energy_bytes_per_s"],
             "%.2f %% of the 6.29 TB/s copy rate: one read of the pool at that rate would take %.4f ms.  The gather moves %.3g bytes/s (kept"
             % (100 * c["energy_share_of_hbm_copy_rate"], c["one_read_of_the_pool_ms"], c["gather_bytes_per_s"]),
             "samples read and written, 2 bytes each).  What bounds either kernel has not been measured - no counter run was made.",
             "", "## Serving: rows of %d samples at 44800 Hz (frames %s), Trimmer(rescaling_max=%g).trim_batch" % (
                 srv["samples_per_row"], srv["frames"], RESCALE), ""]
    for key in [k for k in srv if k.startswith("B")]:
        s = srv[key]
        lines += ["### %s" % key, ""] + head + [_row("trim_batch", s["trim_batch"]), _row("host: read back, numpy per row, copy back", s["host"]),
                                                 _row("denoise_batch", s["denoise_batch"]), _row("infer_batch", s["infer_batch"]), "",
                                                 "host / device %.1f; %.3g bytes/s; %.3f %% of the served batch; kept %s; lengths equal the host "
                                                 "form's: %s; values that differ from it: %d." % (
                                                     s["host_over_device"], s["bytes_per_s"], 100 * s["share_of_served_batch"], s["kept"],
                                                     s["lengths_equal_host_form"], s["values_differing_from_host_form"]), ""]
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
           "corpus": corpus_case(max(2, args.clips // args.divide), args.reps, args.divide), "serving": serving_case(args.reps, args.divide)}
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "trim.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    with open(os.path.join(args.out, "trim.md"), "w") as f:
        f.write(markdown(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
