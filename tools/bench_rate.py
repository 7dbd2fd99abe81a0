#!/usr/bin/env python3
"""Speaking rate and timestamps (text2speech_amd/rate.py, longform.synthesize_long_timed(speed=, timestamps=); csrc/warp.hip)
against what a caller writes without them.  In one process, after warm-up calls, the forms alternating (the order swaps from one repetition to the
next), synchronised around each call, the median of --reps runs; every form's own spread is (max - min) of its runs.

  (a) warp      a mel of 8 x 80 x 1000 (ragged lengths) and one of 1 x 80 x 200 at rate 0.8:
                  warp_mel       rate.warp_mel: two launches, nothing read back
                  eager          index_select + lerp on the device with the float32 coordinate (j + 0.5) r - 0.5, over the padded
                                 batch (it knows no lengths)
                  numpy          read the mel back, interpolate per entry in float64 on the host, upload
                the three are compared before anything is timed (the eager form's float32 coordinate is the difference)
  (b) chain     synthesize_long_timed on tools/bench_longform.py's workload (16 chunks forced to 150 - 400 frames, 512-channel
                WaveGlow, denoiser, batch_size 8) with speed=None, speed=1.0 and speed=0.8
  (c) timing    ... and with timestamps=True, against speed=None without

--none-only runs (b)'s speed=None form alone: with T2S_LIB_PATH pointing at the parent commit's library (build it there, or
`build_variant`-style into build/parent/) that is the parent's figure, taken on the same box in the same job.  --parent-json FILE
puts such a run's result next to this tree's.  Writes <out>/rate_control.json and <out>/rate_control.md and prints the JSON line."""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from text2speech_amd import audio as A, longform as L, synth  # noqa: E402
from text2speech_amd.glow import WaveGlow  # noqa: E402
from text2speech_amd.tacotron import Tacotron  # noqa: E402
from tools import bench_longform as BL  # noqa: E402

DEV = BL.DEV
RATE = 0.8


def eager(mel, rate, n):
    """what a caller writes today on the device: n output frames over the padded batch, float32 coordinates"""
    F = mel.size(2)
    pos = ((torch.arange(n, device=mel.device, dtype=torch.float32) + 0.5) * rate - 0.5).clamp(0, F - 1)
    f0 = pos.floor().long()
    f1 = (f0 + 1).clamp(max=F - 1)
    return torch.lerp(mel.index_select(2, f0), mel.index_select(2, f1), pos - f0)


def by_numpy(mel, lengths, rate, n_of):
    """read back, np.interp's arithmetic per entry in float64, upload"""
    x = mel.cpu().numpy()
    out = np.zeros((x.shape[0], x.shape[1], max(n_of)), dtype=x.dtype)
    for b, (F, n) in enumerate(zip(lengths, n_of)):
        pos = np.clip((np.arange(n) + 0.5) * rate - 0.5, 0, F - 1)
        f0 = np.floor(pos).astype(np.int64)
        f1 = np.minimum(f0 + 1, F - 1)
        a = pos - f0
        out[b, :, :n] = (1 - a) * x[b][:, f0] + a * x[b][:, f1]
    return torch.from_numpy(out).to(mel.device)


def warp_case(lengths, F, reps):
    from text2speech_amd import rate as RT
    gen = torch.Generator().manual_seed(7)
    mel = ((torch.rand(len(lengths), 80, F, generator=gen) - 0.5) * 8).to(DEV)
    n_of = [RT.warped_length(f, RATE) for f in lengths]
    n_pad = RT.warped_length(F, RATE)
    got = RT.warp_mel(mel, lengths, RATE)
    ref = by_numpy(mel, lengths, RATE, n_of)
    eag = eager(mel, RATE, n_pad)
    diff_np = max(float((got.mel[b, :, :n] - ref[b, :, :n]).abs().max()) for b, n in enumerate(n_of))
    diff_eager = float((got.mel[0, :, :n_of[0]] - eag[0, :, :n_of[0]]).abs().max()) if lengths[0] == F else None
    assert diff_np < 1e-5, diff_np
    res = BL._time({"warp_mel": lambda: RT.warp_mel(mel, lengths, RATE), "eager": lambda: eager(mel, RATE, n_pad),
                    "numpy": lambda: by_numpy(mel, lengths, RATE, n_of)}, reps)
    res.update(shape=[len(lengths), 80, F], frames_out=n_of, max_abs_diff_numpy=diff_np, max_abs_diff_eager_entry0=diff_eager)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=16)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--divide", type=int, default=1)
    ap.add_argument("--none-only", action="store_true")
    ap.add_argument("--parent-json", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--name", default="rate_control")
    args = ap.parse_args()
    taco = Tacotron(synth.TACOTRON_HPARAMS, 80, num_speakers=2)
    taco.load_state_dict(synth.tacotron_state())
    taco = taco.to(DEV).eval()
    wg = WaveGlow(**synth.WAVEGLOW_DEFAULT)
    wg.load_state_dict(synth.waveglow_state())
    wg = wg.to(DEV).eval()
    den = A.Denoiser(wg)
    chunks = BL.make_chunks(args.chunks)
    counts = [L.n_symbols(c) for c in chunks]
    frames_of = {k: max(3, round((150 + (k - 40) * 250 / 88) / args.divide)) for k in counts}
    forced = BL.Forced(taco, frames_of)
    frames = [frames_of[k] for k in counts]
    out = {"chunks": len(chunks), "frames": frames, "rate": RATE, "library": os.environ.get("T2S_LIB_PATH") or "this tree's"}

    def long(**kw):
        return L.synthesize_long_timed(forced, wg, chunks=chunks, seed=BL.SEED, sigma=BL.SIGMA, batch_size=8, denoiser=den,
                                       pause_ms=BL.PAUSE_MS, fade_ms=0, **kw)

    with contextlib.redirect_stderr(io.StringIO()):             # (the max-decoder-steps warning of every call)
        if args.none_only:
            out["chain"] = BL._time({"speed_none": long}, args.reps)
        else:
            from text2speech_amd import rate as RT
            out["warp"] = {"8x80x1000": warp_case([1000, 950, 900, 800, 700, 600, 450, 300], 1000, args.reps),
                           "1x80x200": warp_case([200], 200, args.reps)}
            none, one, slow = long(), long(speed=1.0), long(speed=RATE)
            assert torch.equal(none.audio, one.audio) and torch.equal(none.length, one.length), "speed=1.0 is not speed=None"
            slow_frames = [RT.warped_length(f, RATE) for f in frames]
            pauses = (len(chunks) - 1) * L.ms_to_samples(BL.PAUSE_MS, L.SAMPLING_RATE)
            assert int(none.length) == 256 * sum(frames) + pauses and int(slow.length) == 256 * sum(slow_frames) + pauses
            timed = long(timestamps=True)
            assert torch.equal(timed.audio, none.audio) and int(timed.spans.max()) <= int(none.length)
            out["frame_ratio"] = round(sum(slow_frames) / sum(frames), 4)
            out["chain"] = BL._time({"speed_none": long, "speed_1.0": lambda: long(speed=1.0), "speed_0.8": lambda: long(speed=RATE),
                                     "none_timestamps": lambda: long(timestamps=True),
                                     "0.8_timestamps": lambda: long(speed=RATE, timestamps=True)}, args.reps)
    if args.parent_json:
        with open(args.parent_json) as f:
            out["parent"] = json.load(f)["chain"]["speed_none"]
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, args.name + ".json"), "w") as f:
        json.dump(out, f, indent=1)
    if not args.none_only:
        with open(os.path.join(args.out, args.name + ".md"), "w") as f:
            f.write(markdown(out))
    print(json.dumps(out))


def _row(k, s, extra=""):
    return "| %s | %.3f | %.3f | %.3f | %.3f |%s" % (k, s["median_ms"], s["min_ms"], s["max_ms"], s["spread_ms"], extra)


def markdown(o):
    runs = o["chain"]["speed_none"]["runs"]
    rows = ["# Speaking rate and timestamps: measurements", "",
            "`python tools/bench_rate.py` on one MI355X: one process, warm, the forms alternating, synchronised around each call,",
            "median of %d runs; spread = max - min of a form's own runs.  Synthetic weights, f32." % runs, "",
            "## (a) `warp_mel` at rate %.1f against the eager device form and the host round trip" % o["rate"], ""]
    for name, w in o["warp"].items():
        rows += ["Mel %s, %s -> %s frames:" % (name, "ragged" if len(w["frames_out"]) > 1 else "one entry", w["frames_out"]), "",
                 "| form | median ms | min | max | spread | against warp_mel |", "|---|---|---|---|---|---|"]
        for k in ("warp_mel", "eager", "numpy"):
            rows.append(_row(k, w[k], " %.2fx |" % (w[k]["median_ms"] / w["warp_mel"]["median_ms"])))
        for k in ("eager", "numpy"):
            d = w[k]["median_ms"] - w["warp_mel"]["median_ms"]
            real = abs(d) > 2 * w[k]["spread_ms"]
            apart = w[k]["min_ms"] > w["warp_mel"]["max_ms"]
            rows.append("%s%s is %+.3f ms from warp_mel, %s twice its own spread (%.3f ms): %s." % (
                "" if k == "numpy" else "\n", k, d, "beyond" if real else "inside", 2 * w[k]["spread_ms"],
                ("warp_mel is %s" % ("quicker" if d > 0 else "SLOWER")) if real else
                ("by that rule no difference, though its quickest run (%.3f) is slower than warp_mel's slowest (%.3f)"
                 % (w[k]["min_ms"], w["warp_mel"]["max_ms"])) if apart else "no difference that this measurement can show"))
        rows += ["Largest difference to the host's float64 interpolation %.2e%s." % (
            w["max_abs_diff_numpy"], "" if w["max_abs_diff_eager_entry0"] is None else
            "; to the eager form (float32 coordinate) on entry 0 %.2e" % w["max_abs_diff_eager_entry0"]), ""]
    base = o["chain"]["speed_none"]
    rows += ["## (b), (c) `synthesize_long_timed`, batch_size 8, denoiser: %d chunks of %d - %d frames" % (o["chunks"], min(o["frames"]),
                                                                                                  max(o["frames"])), "",
             "| form | median ms | min | max | spread | against speed=None |", "|---|---|---|---|---|---|"]
    for k in ("speed_none", "speed_1.0", "speed_0.8", "none_timestamps", "0.8_timestamps"):
        rows.append(_row(k, o["chain"][k], " %.3fx |" % (o["chain"][k]["median_ms"] / base["median_ms"])))
    rows += ["", "At rate %.1f the vocoder makes %.4f times the frames; the chain took %.3f times speed=None's median."
             % (o["rate"], o["frame_ratio"], o["chain"]["speed_0.8"]["median_ms"] / base["median_ms"])]
    if "parent" in o:
        p = o["parent"]
        d = base["median_ms"] - p["median_ms"]
        rows += ["", "speed=None under the parent commit's library, in a process of its own in the same job: median %.3f ms (min %.3f, "
                 "max %.3f, spread %.3f)." % (p["median_ms"], p["min_ms"], p["max_ms"], p["spread_ms"]),
                 "This tree's differs by %+.3f ms, %s twice the parent's own spread (%.3f ms): %s."
                 % (d, "inside" if abs(d) <= 2 * p["spread_ms"] else "OUTSIDE", 2 * p["spread_ms"],
                    "unchanged" if abs(d) <= 2 * p["spread_ms"] else "changed")]
    rows += ["", "A difference counts as real only beyond twice the baseline's own spread.  Not measured: trained checkpoints, `.half()`",
             "models, per-symbol tables, rates other than %.1f." % o["rate"], ""]
    return "\n".join(rows)


if __name__ == "__main__":
    main()
