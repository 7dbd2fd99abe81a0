#!/usr/bin/env python3
"""The alignment check (text2speech_amd/alignment.py, csrc/align.hip) against what a caller does without it, and what it adds to
long-form synthesis.  In one process, after warm-up calls, the forms alternating (the order swaps from one repetition to the next),
synchronised around each call, the median of --reps runs; every form's own spread is (max - min) of its runs.

  (a) report    alignment_report on seeded softmax rows already in HBM, at B = 8, N = 1000, T_in = 128 and at B = 1, N = 200,
                T_in = 40, ragged lengths, against
                  host_restatement   the alignments read back and tests/align_ref.py run on them (the baseline)
                  read_back          the read-back alone: the floor of anything the host could do
                The device's report is compared with the restatement before anything is timed.
  (b) chain     synthesize_long on tools/bench_longform.py's workload (batch_size 8, denoiser, fade 0) without a check, and with
                a check whose thresholds are all switched off: nothing is retried, the report and the wider read are what is added.
Writes <out>/align_check.json and <out>/align_check.md and prints the JSON line.  --divide N: N times fewer frames per chunk."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import align_ref as AR  # noqa: E402
from text2speech_amd import alignment as AL, audio as A, longform as L, synth  # noqa: E402
from text2speech_amd.glow import WaveGlow  # noqa: E402
from text2speech_amd.tacotron import Tacotron  # noqa: E402
from tools import bench_longform as BL  # noqa: E402

DEV = BL.DEV
CHECK = AL.AlignmentCheck(skip_max=1, back_max=1, stall_max=3, end_slack=2, min_focus=0.4, max_frames=0)
ALL_OFF = AL.AlignmentCheck(skip_max=-1, back_max=-1, stall_max=-1, end_slack=-1, min_focus=0.0, max_frames=0)


def report_case(B, N, T, reps):
    host = AR.random_alignments(B, N, T, np.float32, 1000 + B)
    rng = np.random.RandomState(B)
    in_len = [T] + [int(v) for v in rng.randint(T // 2, T + 1, B - 1)]
    out_len = [N] + [int(v) for v in rng.randint(N // 2, N + 1, B - 1)]
    a = torch.from_numpy(host).to(DEV)
    in_d, out_d = torch.tensor(in_len, dtype=torch.int32).to(DEV), torch.tensor(out_len, dtype=torch.int32).to(DEV)
    thr = dict(zip(("max_frames", "skip_max", "back_max", "stall_max", "end_slack", "min_focus"), CHECK.thresholds()))
    got = AL.alignment_report(a, in_d, out_d, CHECK)
    want = AR.report(host, in_len, out_len, **thr)
    assert got.path.cpu().tolist() == want.pos.tolist() and got.stats.cpu().tolist() == want.stats.tolist()
    assert got.flags.cpu().tolist() == want.flags.tolist() and got.durations.cpu().tolist() == want.dur.tolist()
    assert all(abs(g - w) <= AR.focus_bound(p, int(s[0])) for g, w, p, s in zip(got.focus.cpu().tolist(), want.focus, want.peak, want.stats))
    out = BL._time({"alignment_report": lambda: AL.alignment_report(a, in_d, out_d, CHECK),
                    "host_restatement": lambda: AR.report(a.cpu().numpy(), in_len, out_len, **thr),
                    "read_back": lambda: a.cpu()}, reps)
    out.update(B=B, N=N, T_in=T, bytes=a.numel() * 4, flags=want.flags.tolist())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=16)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--divide", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    out = {"report": [report_case(8, 1000, 128, args.reps), report_case(1, 200, 40, args.reps)]}
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
    out.update(chunks=len(chunks), symbols=counts, frames=[frames_of[k] for k in counts])

    def long(check):
        return L.synthesize_long(forced, wg, chunks=chunks, seed=BL.SEED, sigma=BL.SIGMA, batch_size=8, denoiser=den,
                                 pause_ms=BL.PAUSE_MS, fade_ms=0, check=check)

    with contextlib.redirect_stderr(io.StringIO()):             # (the max-decoder-steps warning of every call)
        plain, checked = long(None), long(ALL_OFF)
        assert torch.equal(plain.audio, checked.audio) and torch.equal(plain.offsets, checked.offsets)
        assert checked.flags.cpu().tolist() == [0] * len(chunks) and checked.attempts.tolist() == [0] * len(chunks)
        assert checked.stats[:, 0].cpu().tolist() == [frames_of[k] for k in counts]
        out["chain"] = BL._time({"no_check": lambda: long(None), "check_all_off": lambda: long(ALL_OFF)}, args.reps)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "align_check.json"), "w") as f:
        json.dump(out, f, indent=1)
    with open(os.path.join(args.out, "align_check.md"), "w") as f:
        f.write(markdown(out))
    print(json.dumps(out))


def markdown(o):
    runs = o["chain"]["no_check"]["runs"]
    rows = ["# The alignment check: measurements", "",
            "`python tools/bench_align_check.py` on one MI355X: one process, warm, the forms alternating, synchronised around each call,",
            "median of %d runs; spread = max - min of a form's own runs.  Synthetic weights." % runs, "",
            "## (a) the report alone: alignments already in HBM, f32, ragged lengths", ""]
    for r in o["report"]:
        rows += ["B = %d, N = %d, T_in = %d (%.2f MB of alignments):" % (r["B"], r["N"], r["T_in"], r["bytes"] / 1e6), "",
                 "| form | median ms | min | max | spread |", "|---|---|---|---|---|"]
        for k in ("alignment_report", "host_restatement", "read_back"):
            s = r[k]
            rows.append("| %s | %.3f | %.3f | %.3f | %.3f |" % (k, s["median_ms"], s["min_ms"], s["max_ms"], s["spread_ms"]))
        rows.append("")
    rows += ["`host_restatement` is the baseline: the alignments read back and tests/align_ref.py run on them, a Python",
             "loop over the rows - a vectorised host version would be faster, but not faster than `read_back`, the copy alone."]
    for r in o["report"]:
        if r["read_back"]["median_ms"] < r["alignment_report"]["median_ms"]:
            rows.append("At B = %d, N = %d, T_in = %d the copy alone (%.3f ms) is quicker than the report (%.3f ms): two launches and a "
                        "memset are launch-bound at that size, and a host method still has its arithmetic to do behind the copy."
                        % (r["B"], r["N"], r["T_in"], r["read_back"]["median_ms"], r["alignment_report"]["median_ms"]))
    rows += ["",
             "## (b) synthesize_long, batch_size 8, denoiser, %d chunks of %d - %d symbols forced to %d - %d frames"
             % (o["chunks"], min(o["symbols"]), max(o["symbols"]), min(o["frames"]), max(o["frames"])), "",
             "| form | median ms | min | max | spread |", "|---|---|---|---|---|"]
    for k in ("no_check", "check_all_off"):
        s = o["chain"][k]
        rows.append("| %s | %.2f | %.2f | %.2f | %.2f |" % (k, s["median_ms"], s["min_ms"], s["max_ms"], s["spread_ms"]))
    base, chk = o["chain"]["no_check"], o["chain"]["check_all_off"]
    diff = chk["median_ms"] - base["median_ms"]
    real = abs(diff) > 2 * base["spread_ms"]
    rows += ["", "The check adds %+.2f ms to the median (%+.2f %%); twice the spread of the form without a check is %.2f ms, so this %s."
             % (diff, 100 * diff / base["median_ms"], 2 * base["spread_ms"],
                "counts as a real difference" if real else "is no difference that this measurement can show"),
             "With every threshold off nothing is retried: what is added is the two launches and the memset of the report per group,",
             "the cast of its flags and the stack that makes the group's read-back one copy of both.  Not measured: trained checkpoints,",
             "the cost of a retry (a second decode of the rejected chunks, by construction), `.half()` models.", ""]
    return "\n".join(rows)


if __name__ == "__main__":
    main()
