#!/usr/bin/env python3
"""Training batches built on the device from an int16 pool (text2speech_amd/data.py) against the same batches assembled on the host the
reference's way - slice, zero pad and `/ 32768` in CPU torch per item, one `.cuda()` of the padded batch - and then pushed through the
same device mel calls.  Synthetic int16 clips, seeded; in one process, after warm-up calls, the two forms alternating (the order swaps
from one repetition to the next), synchronised around each call:
  mel2samp   Mel2SampBatch at the waveglow/config.json shape: B = 8 segments of 16000 samples, STFT 1024 / 256 / 1024 at 22050 Hz,
             clips of 1 to 4 s (one of them shorter than a segment)
  textmel    TextMelBatch at B = 32, clips spread over 2 to 10 s at the hparams.py rate (44800 Hz), STFT 1024 / 256 / 1024, 80 mels,
             texts of 20 to 150 symbols; host form: the padded [B, T'] floats, the padded texts, the gate rows written in a Python loop
Both forms draw the same crops and must give the same tensors bit for bit, which is checked before anything is timed.
Prints one JSON line: per case the median, least and greatest ms per batch of each form and host / device."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from text2speech_amd import data  # noqa: E402

DEV = "cuda:0"


def _once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _stats(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def _time(runs, reps):
    for fn in runs.values():
        fn()
        fn()
    ms = {k: [] for k in runs}
    order = list(runs)
    for r in range(reps):
        for k in (order if r % 2 == 0 else order[::-1]):
            ms[k].append(_once(runs[k]))
    st = {k: _stats(v) for k, v in ms.items()}
    st["host_over_device"] = round(st["host"]["median_ms"] / st["device"]["median_ms"], 2)
    return st


def mel2samp_case(reps):
    sr, seg, B = 22050, 16000, 8
    gen = np.random.RandomState(1)
    lens = [int(sr * s) for s in np.linspace(1.0, 4.0, 15)] + [seg - 1000]
    clips = [gen.randint(-20000, 20000, n).astype(np.int16) for n in lens]
    pool = data.PcmPool(clips, sr, DEV)
    loader = data.Mel2SampBatch(pool, seg, 1024, 256, 1024, sr, 0.0, 8000.0)
    pick = random.Random(5)
    batches = [[pick.randrange(len(clips)) for _ in range(B)] for _ in range(4)]
    batches[0][3] = len(clips) - 1                                  # the short clip
    state = {"n": 0}

    def host_form(indices, starts):
        rows = []
        for i, s in zip(indices, starts):
            a = torch.from_numpy(clips[i]).float()
            a = a[s:s + seg] if a.size(0) >= seg else torch.nn.functional.pad(a, (0, seg - a.size(0)), "constant")
            rows.append(a / 32768.0)
        audio = torch.stack(rows).to(DEV)
        return loader.stft._mel(audio)[0], audio

    def device():
        state["n"] += 1
        return loader(batches[state["n"] % len(batches)])

    def host():
        state["n"] += 1
        idx = batches[state["n"] % len(batches)]
        return host_form(idx, data.crop_starts([len(clips[i]) for i in idx], seg, loader.rng))

    mel, audio = loader(batches[0])
    mel_h, audio_h = host_form(batches[0], loader.last_starts)
    assert torch.equal(audio, audio_h) and torch.equal(mel, mel_h), "the two forms differ"
    out = _time({"device": device, "host": host}, reps)
    out.update(B=B, segment_length=seg, stft="1024/256/1024", sampling_rate=sr, pool_samples=int(pool.pcm.numel()))
    return out


def textmel_case(reps):
    sr, B, hop = 44800, 32, 256
    gen = np.random.RandomState(2)
    lens = [int(sr * s) for s in np.linspace(2.0, 10.0, 48)]
    gen.shuffle(lens)
    clips = [gen.randint(-20000, 20000, n).astype(np.int16) for n in lens]
    seqs = [gen.randint(2, 80, gen.randint(20, 151)).tolist() for _ in clips]
    pool = data.PcmPool(clips, sr, DEV)
    loader = data.TextMelBatch(pool, seqs, 1, 1024, hop, 1024, 80, sr, 0.0, 8000.0)
    pick = random.Random(6)
    batches = [pick.sample(range(len(clips)), B) for _ in range(4)]
    state = {"n": 0}

    def host_form(indices):
        input_lengths, order = torch.sort(torch.LongTensor([len(seqs[i]) for i in indices]), dim=0, descending=True)
        idx = [indices[k] for k in order.tolist()]
        text = torch.zeros(B, int(input_lengths[0]), dtype=torch.int64)
        for k, i in enumerate(idx):
            text[k, :len(seqs[i])] = torch.LongTensor(seqs[i])
        n = torch.tensor([len(clips[i]) for i in idx])
        t_out = 1 + int(n.max()) // hop
        width = data.gather_width(int(n.max()), t_out, hop)
        y = torch.zeros(B, width)
        gate = torch.zeros(B, t_out)
        for k, i in enumerate(idx):
            y[k, :len(clips[i])] = torch.from_numpy(clips[i]).float() / 32768.0
            gate[k, len(clips[i]) // hop:] = 1
        mel, frames = loader.stft._mel(y.to(DEV), n)
        return text.to(DEV), input_lengths, mel, gate.to(DEV), torch.zeros(B).to(DEV), frames.to(DEV)

    def device():
        state["n"] += 1
        return loader.collate(batches[state["n"] % len(batches)])

    def host():
        state["n"] += 1
        return host_form(batches[state["n"] % len(batches)])

    for g, h in zip(loader.collate(batches[0]), host_form(batches[0])):
        assert torch.equal(g, h), "the two forms differ"
    out = _time({"device": device, "host": host}, reps)
    out.update(B=B, clip_seconds=[2.0, 10.0], stft="1024/256/1024", sampling_rate=sr, pool_samples=int(pool.pcm.numel()),
               frames=[1 + int(max(len(clips[i]) for i in b)) // hop for b in batches])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X: a time taken elsewhere says nothing"
    out = {"reps": args.reps, "torch_threads": torch.get_num_threads(), "mel2samp": mel2samp_case(args.reps),
           "textmel": textmel_case(args.reps)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
