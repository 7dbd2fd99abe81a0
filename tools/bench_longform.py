#!/usr/bin/env python3
"""Long-form synthesis (text2speech_amd/longform.py, audio.join_batches; csrc/join.hip) against what a caller writes without it.
Synthetic weights, a 512-channel WaveGlow, --chunks chunks of 40 - 128 symbols (all counts different), each FORCED to a frame count
of its own between 150 and 400, growing with its symbols: the decoder never stops by itself (gate threshold 2), a group decodes as
many steps as its longest chunk needs - what a real batch does - and the output lengths are then set to the forced ones, on the
device.  In one process, after warm-up calls, the forms alternating (the order swaps from one repetition to the next), synchronised
around each call, the median of --reps runs; every form's own spread is (max - min) of its runs.

  (a) join      the rows of the batch_size-8 groups (denoised), already in HBM:
                  join_batches   audio.join_batches over the groups: nothing is read back
                  host_cat       what a caller writes today: the lengths read back, Python slices, torch.cat with zero tensors
                the two results must be equal sample for sample (fade 0), which is checked before anything is timed
  (b) chain     synthesize_long at batch_size 1, 4 and 8 (denoiser, fade 0) against
                  solo_loop      per chunk inference(seed) -> infer(seed) -> denoiser, then the same host concatenation
Writes <out>/longform.json and <out>/longform.md and prints the JSON line.  --divide N: N times fewer frames per chunk."""
import argparse
import contextlib
import io
import json
import os
import random
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from text2speech_amd import audio as A, longform as L, synth  # noqa: E402
from text2speech_amd.glow import WaveGlow  # noqa: E402
from text2speech_amd.tacotron import Tacotron  # noqa: E402

DEV = "cuda:0"
SEED, SIGMA, PAUSE_MS = 20240611, 0.666, 250.0
SYLLABLES = "가나다라마바사아자차카타파하고노도로모보소오조초코토포호"


def _once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _stats(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "spread_ms": round(max(ms) - min(ms), 3), "runs": len(ms)}


def _time(runs, reps):
    for fn in runs.values():
        fn()
    ms = {k: [] for k in runs}
    order = list(runs)
    for r in range(reps):
        for k in (order if r % 2 == 0 else order[::-1]):
            ms[k].append(_once(runs[k]))
    return {k: _stats(v) for k, v in ms.items()}


def make_chunks(n, lo=40, hi=128, seed=3):
    """n strings of open syllables (two ids each) and spaces with n different id counts spread over [lo, hi], shuffled"""
    rng = random.Random(seed)
    counts = sorted({lo + round(i * (hi - lo) / max(1, n - 1)) for i in range(n)})
    assert len(counts) == n
    chunks = []
    for c in counts:
        s, k = "", 0
        while L.n_symbols(s + ".") < c:
            left = c - L.n_symbols(s + ".")
            if left == 1:
                s += ","                                        # one id
            elif k % 4 == 3 and left >= 3:
                s += " " + rng.choice(SYLLABLES)                # three ids
                k += 1
            else:
                s += rng.choice(SYLLABLES)                      # an open syllable: two ids
                k += 1
        chunks.append(s + ".")
    got = [L.n_symbols(c) for c in chunks]
    assert len(set(got)) == n, got
    rng.shuffle(chunks)
    return chunks


class Forced:
    """A Tacotron whose chunk of k ids always yields frames_of[k] frames: threshold 2, max_decoder_steps the call's longest, then
    the output lengths replaced - from a table that lives on the device, indexed without a read-back."""

    def __init__(self, model, frames_of):
        self.m, self.frames_of = model, frames_of
        self.table = torch.zeros(max(frames_of) + 1, dtype=torch.int64)
        for k, f in frames_of.items():
            self.table[k] = f
        self.table = self.table.to(DEV)
        self.decoder = model.decoder
        self.training = False

    def _steps(self, counts):
        self.m.decoder.gate_threshold = 2.0
        self.m.decoder.max_decoder_steps = max(self.frames_of[int(k)] for k in counts)

    def inference_batch(self, ids, lengths, seeds=None):
        self._steps(lengths.tolist())
        out = self.m.inference_batch(ids, lengths, seeds=seeds)
        self.m.decoder.max_decoder_steps = 1 << 30              # (synthesize_long's `truncated` compares with it: nothing is flagged)
        return out[:4] + [self.table[A._to_device(lengths.to(torch.int64), DEV)]]

    def inference(self, ids, seed):
        self._steps([ids.size(1)])
        return self.m.inference(ids, None, seed=seed)


def host_cat(batches, order, gaps):
    """today's way: read the lengths back, slice, concatenate with zero tensors"""
    rows = []
    for audio, lengths in batches:
        a = audio.reshape(-1, audio.size(-1))
        for b in range(a.size(0)):
            rows.append(a[b, :int(lengths[b])])
    parts = []
    for p, r in enumerate(order):
        parts.append(rows[r].float())
        if p < len(order) - 1 and gaps[p]:
            parts.append(torch.zeros(gaps[p], dtype=torch.float32, device=rows[r].device))
    return torch.cat(parts)[None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=16)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--divide", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    taco = Tacotron(synth.TACOTRON_HPARAMS, 80, num_speakers=2)
    taco.load_state_dict(synth.tacotron_state())
    taco = taco.to(DEV).eval()
    wg = WaveGlow(**synth.WAVEGLOW_DEFAULT)
    wg.load_state_dict(synth.waveglow_state())
    wg = wg.to(DEV).eval()
    den = A.Denoiser(wg)
    chunks = make_chunks(args.chunks)
    counts = [L.n_symbols(c) for c in chunks]
    frames_of = {k: max(3, round((150 + (k - 40) * 250 / 88) / args.divide)) for k in counts}
    forced = Forced(taco, frames_of)
    n = len(chunks)
    seeds = L.chunk_seeds(SEED, n)
    pause = L.ms_to_samples(PAUSE_MS, L.SAMPLING_RATE)
    out = {"chunks": n, "symbols": counts, "frames": [frames_of[k] for k in counts], "pause_samples": pause,
           "audio_seconds": round(sum(frames_of[k] for k in counts) * 256 / L.SAMPLING_RATE + (n - 1) * PAUSE_MS / 1e3, 2)}

    def long(bs):
        return L.synthesize_long(forced, wg, chunks=chunks, seed=SEED, sigma=SIGMA, batch_size=bs, denoiser=den, pause_ms=PAUSE_MS,
                                 fade_ms=0)

    def solo_loop():
        parts = []
        for i, c in enumerate(chunks):
            ids = torch.from_numpy(L.text_to_sequence(c)).to(torch.int64)[None].to(DEV)
            a = den(wg.infer(forced.inference(ids, seeds[i])[1], sigma=SIGMA, seed=seeds[i]), 0.1)[:, 0]
            parts.append(a[0])
            if i < n - 1:
                parts.append(torch.zeros(pause, dtype=torch.float32, device=DEV))
        return torch.cat(parts)[None]

    with contextlib.redirect_stderr(io.StringIO()):             # (the max-decoder-steps warning of every call)
        # ---- (a): the join alone, on the rows of the batch_size-8 groups
        groups, order = L._plan(counts, 8, True)
        batches = []
        for g in groups:
            ids = torch.zeros(len(g), max(counts[c] for c in g), dtype=torch.int64)
            for b, c in enumerate(g):
                ids[b, :counts[c]] = torch.from_numpy(L.text_to_sequence(chunks[c])).to(torch.int64)
            res = forced.inference_batch(ids.to(DEV), torch.tensor([counts[c] for c in g]), seeds=[seeds[c] for c in g])
            frames = res[4].cpu()
            wav, _ = wg.infer_batch(res[1], frames, sigma=SIGMA, seeds=[seeds[c] for c in g])
            batches.append(den.denoise_batch(wav, frames * 256, 0.1))
        gaps = [pause] * (n - 1)
        joined, length, offsets = A.join_batches(batches, order=order, pauses=gaps, fade=0)
        want = host_cat(batches, order, gaps)
        assert int(length) == want.size(1) and torch.equal(joined[:, :want.size(1)], want) and not bool(joined[:, want.size(1):].any())
        out["join"] = _time({"join_batches": lambda: A.join_batches(batches, order=order, pauses=gaps, fade=0),
                             "host_cat": lambda: host_cat(batches, order, gaps)}, args.reps)
        out["join"]["samples"] = int(length)
        out["join"]["cap"] = joined.size(1)
        # ---- (b): the whole chain
        ref = solo_loop()
        for bs in (1, 4, 8):
            r = long(bs)
            k = int(r.length)
            # (the samples are compared by the tests, with chunks that stop by themselves: a forced length cuts the batched mel
            # behind the postnet, whose last frames then saw what lay behind the cut)
            assert k == ref.size(1) and bool(torch.isfinite(r.audio).all()), (k, ref.size(1))
        out["chain"] = _time({"solo_loop": solo_loop, "batch_size_1": lambda: long(1), "batch_size_4": lambda: long(4),
                              "batch_size_8": lambda: long(8)}, args.reps)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "longform.json"), "w") as f:
        json.dump(out, f, indent=1)
    with open(os.path.join(args.out, "longform.md"), "w") as f:
        f.write(markdown(out))
    print(json.dumps(out))


def markdown(o):
    rows = ["# Long-form synthesis: measurements", "",
            "`python tools/bench_longform.py` on one MI355X: one process, warm, the forms alternating, synchronised around each call,",
            "median of %d runs; spread = max - min of a form's own runs.  Synthetic weights, 512-channel WaveGlow, f32, %d chunks of"
            % (o["join"]["join_batches"]["runs"], o["chunks"]),
            "%d - %d symbols forced to %d - %d frames (%.1f s of audio with the %d-sample pauses)."
            % (min(o["symbols"]), max(o["symbols"]), min(o["frames"]), max(o["frames"]), o["audio_seconds"], o["pause_samples"]), "",
            "## (a) the join alone: %d samples into a row of %d" % (o["join"]["samples"], o["join"]["cap"]), "",
            "| form | median ms | min | max | spread |", "|---|---|---|---|---|"]
    for k in ("join_batches", "host_cat"):
        s = o["join"][k]
        rows.append("| %s | %.3f | %.3f | %.3f | %.3f |" % (k, s["median_ms"], s["min_ms"], s["max_ms"], s["spread_ms"]))
    rows += ["", "## (b) the chain: text to the joined utterance, denoiser included", "",
             "| form | median ms | min | max | spread | against solo_loop |", "|---|---|---|---|---|---|"]
    base = o["chain"]["solo_loop"]
    for k in ("solo_loop", "batch_size_1", "batch_size_4", "batch_size_8"):
        s = o["chain"][k]
        rows.append("| %s | %.2f | %.2f | %.2f | %.2f | %.2fx |"
                    % (k, s["median_ms"], s["min_ms"], s["max_ms"], s["spread_ms"], base["median_ms"] / s["median_ms"]))
    rows += ["", "A difference counts as real only beyond twice the baseline's own spread (%.3f ms for host_cat, %.2f ms for solo_loop)."
             % (o["join"]["host_cat"]["spread_ms"], base["spread_ms"]),
             "What batching gains in (b) is the Tacotron decode, whose steps serve a whole group; the f32 vocoder batch also computes its",
             "padding and gains nothing on mels this long (README, \"Batched vocoding of ragged mels\").  A forced length cuts a batched mel",
             "behind the postnet, so the samples are not compared here: tests/test_longform_gpu.py does that with chunks that stop by",
             "themselves.  Not measured: trained checkpoints, real paragraph-length distributions, `.half()` models.", ""]
    return "\n".join(rows)


if __name__ == "__main__":
    main()
