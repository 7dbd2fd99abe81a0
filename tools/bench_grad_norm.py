#!/usr/bin/env python3
"""What the gradient norm costs on one MI355X, warm, with device events, in one process:

(a) t2s_grad_norm_table alone, and t2s_adam_table on the same table for comparison, over the job tables of the Tacotron-2 model and
    of the 512-channel WaveGlow (one gradient tensor per parameter, as the optimizer sees them): microseconds, bytes / time, share of
    the measured HBM rate;
(b) the Tacotron-2 train step of tools/bench_tacotron_train.py three ways, alternating: FusedAdam as it was (max_grad_norm=None),
    FusedAdam(max_grad_norm=1.0), and plain FusedAdam preceded by torch.nn.utils.clip_grad_norm_ - with the first one's own
    run-to-run spread beside the differences.

Writes profiles/grad_norm.json (or --out).  Nothing here is asserted by a test."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from text2speech_amd import _lib, synth  # noqa: E402
from text2speech_amd.optim import FusedAdam  # noqa: E402

HBM_MEASURED_TBS = 6.29       # MI355X float4 copy (8.0 TB/s spec)
HBM_SPEC_TBS = 8.0


def _timed(fn, iters, flush=None):
    """Median / min / max microseconds of `iters` calls, each between its own pair of events (after two warm calls).  flush: a buffer
    larger than the 256 MB Infinity Cache, overwritten before every timed call so that the call reads from HBM."""
    fn()
    fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        if flush is not None:
            flush.add_(1.0)
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    us = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return dict(median_us=statistics.median(us), min_us=us[0], max_us=us[-1])


def _rate(row, n_bytes):
    tbs = n_bytes / (row["median_us"] * 1e-6) / 1e12
    row.update(bytes=n_bytes, TB_per_s=tbs, share_of_measured_hbm=tbs / HBM_MEASURED_TBS, share_of_spec_hbm=tbs / HBM_SPEC_TBS)
    return row


def table_bench(name, shapes, iters):
    """One f32 gradient (and parameter, and two moments) per shape, allocated one by one as a model's are."""
    gen = torch.Generator(device="cuda").manual_seed(1)
    grads = [torch.randn(s, device="cuda", generator=gen) * 1e-2 for s in shapes]
    ps = [torch.zeros_like(g) for g in grads]
    ms = [torch.zeros_like(g) for g in grads]
    vs = [torch.zeros_like(g) for g in grads]
    rows, blk, vec = [], 0, 0
    for p, g, m, v in zip(ps, grads, ms, vs):
        rows.append([p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), g.numel(), blk])
        blk += -(-g.numel() // 1024)
        vec += g.numel() // 1024 if g.data_ptr() % 16 == 0 else 0
    jobs = torch.tensor(rows, dtype=torch.int64).cuda()
    n = sum(g.numel() for g in grads)
    partial = torch.empty(_lib.load().t2s_grad_norm_partials(), dtype=torch.float64, device="cuda")
    out = torch.zeros(4, device="cuda")
    st = _lib.current_stream()
    step = [0]

    def norm():
        _lib.call("t2s_grad_norm_table", _lib.ptr(jobs), len(rows), blk, 1.0, 1.0, _lib.ptr(partial), _lib.ptr(out), st)

    def adam():
        step[0] += 1
        _lib.call("t2s_adam_table", _lib.ptr(jobs), len(rows), blk, 1e-4, 0.9, 0.999, 1e-8, step[0], 1.0, 0.0, st)

    def adam_clip():
        step[0] += 1
        _lib.call("t2s_adam_table_clip", _lib.ptr(jobs), len(rows), blk, 1e-4, 0.9, 0.999, 1e-8, step[0], 1.0, 0.0, _lib.ptr(out), 1, st)

    flush = torch.zeros(256 * 2 ** 20, device="cuda")                          # 1 GiB
    res = dict(table=name, tensors=len(rows), elements=n, table_blocks=blk, float4_blocks=vec,
               grad_norm=_rate(_timed(norm, iters, flush), 4 * n),              # one read of the gradients, from HBM
               grad_norm_back_to_back=_rate(_timed(norm, iters), 4 * n),        # the same with whatever the caches kept
               adam_table=_rate(_timed(adam, iters), 7 * 4 * n),                # reads p g m v, writes p m v
               adam_table_clip=_rate(_timed(adam_clip, iters), 7 * 4 * n))
    want = float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads)))
    res["norm"], res["norm_float64_torch"] = float(out[0]), want
    res["norm_over_adam_rate"] = res["grad_norm"]["TB_per_s"] / res["adam_table"]["TB_per_s"]
    print("[grad_norm] %-9s %4d tensors %10d elements: norm %8.1f us %.2f TB/s (%.0f%% of %.2f) | adam_table %8.1f us %.2f TB/s | "
          "adam_table_clip %8.1f us" % (name, len(rows), n, res["grad_norm"]["median_us"], res["grad_norm"]["TB_per_s"],
                                        100 * res["grad_norm"]["share_of_measured_hbm"], HBM_MEASURED_TBS, res["adam_table"]["median_us"],
                                        res["adam_table"]["TB_per_s"], res["adam_table_clip"]["median_us"]), file=sys.stderr, flush=True)
    return res


def tacotron_step_bench(rounds, steps):
    from text2speech_amd.tacotron import Tacotron
    from text2speech_amd.tacotron.loss_function import Tacotron2Loss
    B, T_in, T_out = 32, 256, 800
    m = Tacotron(dict(synth.TACOTRON_HPARAMS), 80, num_speakers=2)
    m.load_state_dict(synth.tacotron_state())
    m = m.cuda().train()
    params = list(m.parameters())
    gen = torch.Generator().manual_seed(21)
    text = torch.randint(2, 80, (B, T_in), generator=gen).cuda()
    mel = torch.randn(B, 80, T_out, generator=gen).cuda()
    gate = torch.zeros(B, T_out).cuda()
    gate[:, -1] = 1
    il = torch.full((B,), T_in, dtype=torch.long).cuda()
    ol = torch.full((B,), T_out, dtype=torch.long).cuda()
    inp = (text, il, mel, T_in, torch.zeros(B).cuda(), ol)
    crit = Tacotron2Loss()
    plain = FusedAdam(params, lr=1e-4, weight_decay=1e-6)
    clipped = FusedAdam(params, lr=1e-4, weight_decay=1e-6, max_grad_norm=1.0)
    eager = FusedAdam(params, lr=1e-4, weight_decay=1e-6)

    def step(which):
        m.zero_grad(set_to_none=True)
        crit(m(inp), (mel, gate)).backward()
        if which == "eager_clip_then_plain":
            torch.nn.utils.clip_grad_norm_(params, 1.0)
            eager.step()
        elif which == "max_grad_norm_1":
            clipped.step()
        else:
            plain.step()

    variants = ("plain", "max_grad_norm_1", "eager_clip_then_plain")
    for v in variants:
        for _ in range(3):
            step(v)
    torch.cuda.synchronize()
    ms = {v: [] for v in variants}
    for r in range(rounds):
        for v in variants:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                step(v)
            b.record()
            torch.cuda.synchronize()
            ms[v].append(a.elapsed_time(b) / steps)
        print("[grad_norm] tacotron step round %d: " % r + "  ".join("%s %.2f ms" % (v, ms[v][-1]) for v in variants), file=sys.stderr,
              flush=True)
    med = {v: statistics.median(ms[v]) for v in variants}
    return dict(shape="B=32 T_in=256 T_out=800, zero_grad + forward + loss + backward + optimizer", steps_per_round=steps, rounds=rounds,
                ms_per_step=ms, median_ms=med, plain_spread_ms=max(ms["plain"]) - min(ms["plain"]),
                max_grad_norm_1_minus_plain_ms=med["max_grad_norm_1"] - med["plain"],
                eager_clip_minus_plain_ms=med["eager_clip_then_plain"] - med["plain"],
                grad_norm_last=float(clipped.grad_norm), parameters=len(params), elements=sum(p.numel() for p in params))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_norm.json"))
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_grad_norm needs an MI355X"
    _lib.load()
    from text2speech_amd.glow import WaveGlow
    from text2speech_amd.tacotron import Tacotron
    res = dict(hbm_measured_TB_per_s=HBM_MEASURED_TBS, hbm_spec_TB_per_s=HBM_SPEC_TBS, tables=[])
    for name, model in (("tacotron", lambda: Tacotron(dict(synth.TACOTRON_HPARAMS), 80, num_speakers=2)),
                        ("waveglow", lambda: WaveGlow(**synth.WAVEGLOW_DEFAULT))):
        shapes = [tuple(p.shape) for p in model().parameters()]
        res["tables"].append(table_bench(name, shapes, a.iters))
        torch.cuda.empty_cache()
    if not a.no_step:
        res["tacotron_train_step"] = tacotron_step_bench(a.rounds, a.steps)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
