"""The alignment check on the device through its Python surface (text2speech_amd/alignment.py) and inside long-form synthesis
(longform.synthesize_long(check=, max_attempts=)): alignment_report against tests/align_ref.py on what the models return, with no
read-back and on a caller's stream; synthesize_long with retries replayed from its parts, pass by pass, and against the solo chains
of the attempts kept.

The small models and the five chunks of tests/longform_util.py, 40 decoder steps at most.  One gate threshold is chosen over the
gate trajectories of all three attempts' seeds (longform_util.pick_threshold), and the threshold of the check is searched among the
chunks' solo statistics of those attempts (``pick_check``): it sits in a gap, clear of every value by a margin that the measured
batch-to-solo difference of the statistic must not exceed.  Every figure is printed before it is asserted
(profiles/align_check_tests.md records them)."""
import numpy as np
import pytest
import torch

import align_ref as AR
import longform_util as U
import stream_util as SU
import streaming_ref as R
from text2speech_amd import _lib, alignment as AL, audio as A, longform as L

pytestmark = pytest.mark.gpu

DEV = U.DEV
SOLO_BAR = R.SOLO_BAR
STRIDE = 256
RATE = 44800
PAUSE_MS = 2.0
ATTEMPTS = 3
FOCUS_MARGIN = 1e-4                                 # as longform_util.pick_threshold's margin on gate probabilities
OFF = dict(skip_max=-1, back_max=-1, stall_max=-1, end_slack=-1, min_focus=0.0, max_frames=0)
# statistic -> (the AlignmentCheck keyword that bounds it, its flag bit, whether small values pass)
STATISTICS = (("focus", "min_focus", AR.DIFFUSE, False), ("max_skip", "skip_max", AR.SKIP, True),
              ("max_back", "back_max", AR.BACK, True), ("longest_stall", "stall_max", AR.STALL, True))


def thresholds_of(check, max_frames=0):
    return dict(zip(("max_frames", "skip_max", "back_max", "stall_max", "end_slack", "min_focus"), check.thresholds(max_frames)))


def value(rep, b, statistic):
    return float(rep.focus[b]) if statistic == "focus" else int(rep.stats[b, AL.STAT_NAMES.index(statistic)])


def pick_check(solo):
    """solo[k][c]: the restatement's report of chunk c decoded alone at attempt k.  A statistic and a threshold in a gap of its
    values over all chunks and attempts, such that at attempt 0 a chunk passes and a chunk fails -> (statistic, keyword, threshold,
    margin, flags[k][c] the solo values predict).  The float statistic wants FOCUS_MARGIN on either side; an integer one is bounded
    by an integer v (v passes, v + 1 fails), so every value lies at least 1/2 from the boundary v + 1/2.  Fails where there is none:
    the tests must not pass vacuously."""
    n = len(solo[0])
    seen = {}
    for statistic, keyword, bit, small_passes in STATISTICS:
        vals = [[value(solo[k][c], 0, statistic) for c in range(n)] for k in range(ATTEMPTS)]
        seen[statistic] = vals
        flat = sorted({v for row in vals for v in row})
        best = None
        for lo, hi in zip(flat, flat[1:]):
            if statistic == "focus":
                if hi - lo <= 2 * FOCUS_MARGIN:
                    continue
                thr, margin = 0.5 * (lo + hi), FOCUS_MARGIN
            else:
                thr, margin = lo, 0.5
            passes = [[(v <= thr) if small_passes else (v >= thr) for v in row] for row in vals]
            if not (any(passes[0]) and not all(passes[0])):
                continue
            later = sum(1 for c in range(n) if not passes[0][c] and any(passes[k][c] for k in range(1, ATTEMPTS)))
            key = (later > 0, min(sum(passes[0]), n - sum(passes[0])), later)
            if best is None or key > best[0]:
                best = (key, thr, margin, [[0 if p else bit for p in row] for row in passes])
        if best is not None:
            return statistic, keyword, best[1], best[2], best[3]
    raise AssertionError(("no threshold on any statistic makes a chunk pass and a chunk fail at attempt 0", seen))


def pick_gate(probs):
    """One gate threshold for the trajectories of every attempt's seeds, found as longform_util.pick_threshold finds its own (a gap
    of the gate values, every value an entry meets up to its stop step 1e-4 clear of it) but without asking that every entry stops:
    another seed moves a trajectory, and an entry that runs into the 40 steps is a legitimate chunk here (the check's TRUNCATED
    bit is off).  Every entry has MIN_FRAMES frames at least and the first attempt's entries as many different lengths as can be
    had (two at least) -> (threshold, frames of every trajectory)."""
    n = probs[0].numel()
    best, best_key = None, None
    for thr, stops in U._candidates(probs, 1e-4):
        frames = [min(s + 1, n) for s in stops]
        if min(frames) < U.MIN_FRAMES:
            continue
        key = (len(set(frames[:5])), len(set(frames)), -sum(f == n for f in frames))
        if best_key is None or key > best_key:
            best, best_key = (thr, frames), key
    assert best is not None and best_key[0] >= 2, ("no gate threshold gives the first attempt's chunks two different lengths",
                                                   [[round(float(v), 5) for v in p[:12]] for p in probs])
    return best


def _padded(ids, group):
    n_ids = [ids[c].size(1) for c in group]
    padded = torch.zeros(len(group), max(n_ids), dtype=torch.int64)
    for b, c in enumerate(group):
        padded[b, :n_ids[b]] = ids[c][0]
    return padded, n_ids


@pytest.fixture(scope="module")
def case():
    """the models, the seeds of every attempt, the gate threshold, the solo reports and the check they give: computed once"""
    assert torch.cuda.is_available()
    _lib.load()
    t, w = U.tacotron(), U.waveglow()
    seeds = U.seeds()
    table = [[AL.attempt_seeds(s, k) for s in seeds] for k in range(ATTEMPTS)]
    probs = [p for k in range(ATTEMPTS) for p in U.solo_gate_probs(t, table[k])]
    gate, frames = pick_gate(probs)
    print("align-check case: gate threshold %.6f, frames by attempt %s" % (gate, [frames[5 * k:5 * k + 5] for k in range(ATTEMPTS)]))
    ids = U.chunk_ids()
    solo, solo_mel = [], []
    try:
        U.set_decoder(t, gate, U.N_STEPS)
        for k in range(ATTEMPTS):
            outs = [t.inference(i.to(DEV), None, seed=s) for i, s in zip(ids, table[k])]
            solo.append([AR.report(o[3].cpu().numpy(), **AR.OFF) for o in outs])
            solo_mel.append([o[1] for o in outs])
    finally:
        U.restore_decoder(t)
    for k in range(ATTEMPTS):
        for c in range(5):
            r = solo[k][c]
            assert r.stats[0, 0] == frames[5 * k + c]
            print("align-check solo attempt %d chunk %d: stats %s focus %.6f" % (k, c, r.stats[0].tolist(), r.focus[0]))
    statistic, keyword, thr, margin, predicted = pick_check(solo)
    check = AL.AlignmentCheck(**dict(OFF, **{keyword: thr if statistic == "focus" else int(thr)}))
    print("align-check: statistic %s, %s = %r, margin %g, predicted flags by attempt %s" % (statistic, keyword, thr, margin, predicted))
    return dict(t=t, w=w, seeds=seeds, table=table, gate=gate, ids=ids, solo=solo, solo_mel=solo_mel, statistic=statistic,
                margin=margin, predicted=predicted, check=check)


def _long(case, **kw):
    kw.setdefault("pause_ms", PAUSE_MS)
    kw.setdefault("fade_ms", 0)
    kw.setdefault("batch_size", 2)
    try:
        U.set_decoder(case["t"], case["gate"], U.N_STEPS)
        return L.synthesize_long(case["t"], case["w"], chunks=U.CHUNKS, seed=U.SEED, sigma=U.SIGMA, **kw)
    finally:
        U.restore_decoder(case["t"])


def _decode_group(case, group, group_seeds):
    """inference_batch of one group as synthesize_long calls it -> (its outputs, the restatement's report of its alignments under
    the case's check)"""
    t = case["t"]
    padded, n_ids = _padded(case["ids"], group)
    try:
        U.set_decoder(t, case["gate"], U.N_STEPS)
        out = t.inference_batch(padded.to(DEV), torch.tensor(n_ids), seeds=group_seeds)
    finally:
        U.restore_decoder(t)
    rep = AR.report(out[3].cpu().numpy(), n_ids, out[4].cpu().tolist(), **thresholds_of(case["check"], U.N_STEPS))
    return out, rep


def _same_report(got, want, rows=None, label=""):
    """an AlignmentReport (or LongFormChecked) against align_ref's Report: integers equal, focus inside its bound"""
    sel = slice(None) if rows is None else rows
    assert got.flags.dtype == torch.int32 and got.flags.cpu().tolist() == want.flags[sel].tolist(), label
    assert got.stats.dtype == torch.int32 and got.stats.cpu().tolist() == want.stats[sel].tolist(), label
    assert got.durations.dtype == torch.int32 and got.durations.cpu().tolist() == want.dur[sel].tolist(), label
    assert got.focus.dtype == torch.float64
    for g, w, st, pk in zip(got.focus.cpu().tolist(), want.focus[sel], want.stats[sel], want.peak[sel]):
        assert abs(g - w) <= AR.focus_bound(pk, int(st[0])), (label, g, w)


@pytest.mark.parametrize("half", [False, True])
def test_report_on_inference_batch(case, half):
    t = U.tacotron().half() if half else case["t"]
    group = [0, 3, 1, 4, 2]
    padded, n_ids = _padded(case["ids"], group)
    try:
        U.set_decoder(t, case["gate"], U.N_STEPS)
        out = t.inference_batch(padded.to(DEV), torch.tensor(n_ids), seeds=[case["seeds"][c] for c in group])
    finally:
        U.restore_decoder(t)
    align, olen = out[3], out[4]
    assert align.dtype == (torch.float16 if half else torch.float32) and olen.dtype == torch.int64 and olen.is_cuda
    check = AL.AlignmentCheck(skip_max=1, back_max=1, stall_max=3, end_slack=1, min_focus=0.2, max_frames=None)
    want = AR.report(align.cpu().numpy(), n_ids, olen.cpu().tolist(), **thresholds_of(check))
    assert half or len(set(want.stats[:, 0].tolist())) >= 2, "the entries have one length: the ragged tail is not exercised"
    for lens_in, lens_out in ((n_ids, olen), (torch.tensor(n_ids), olen.cpu()), (torch.tensor(n_ids, dtype=torch.int32).to(DEV),
                                                                                 olen.to(torch.int32))):
        got = AL.alignment_report(align, lens_in, lens_out, check)
        assert all(x.is_cuda for x in got)
        _same_report(got, want, label="half %s" % half)
        assert got.path.dtype == torch.int32 and got.path.cpu().tolist() == want.pos.tolist()
    print("alignment_report%s: flags %s, stats %s" % (" (.half())" if half else "", want.flags.tolist(), want.stats.tolist()))
    # a view of wider rows is read where it is; a transposed one is copied: the same report
    wide = torch.full((align.size(0), align.size(1), align.size(2) + 3), float("nan"), dtype=align.dtype, device=DEV)
    wide[:, :, :align.size(2)] = align
    for view in (wide[:, :, :align.size(2)], align.transpose(1, 2).contiguous().transpose(1, 2)):
        assert not view.is_contiguous()
        got = AL.alignment_report(view, n_ids, olen, check)
        _same_report(got, want)
    with pytest.raises(_lib.T2SError, match="float32 or float16"):
        AL.alignment_report(align.double(), n_ids, olen)
    with pytest.raises(_lib.T2SError, match="holds 5 entries"):
        AL.alignment_report(align, n_ids[:4], olen)


def test_report_on_inference_without_lengths(case):
    t = case["t"]
    try:
        U.set_decoder(t, case["gate"], U.N_STEPS)
        align = t.inference(case["ids"][0].to(DEV), None, seed=case["seeds"][0])[3]
    finally:
        U.restore_decoder(t)
    got = AL.alignment_report(align)
    want = AR.report(align.cpu().numpy(), **thresholds_of(AL.AlignmentCheck()))
    _same_report(got, want)
    assert got.stats[0, :2].tolist() == [align.size(1), align.size(2)]
    assert got.path.cpu().tolist() == want.pos.tolist() and int(got.durations.sum()) == align.size(1)


def test_report_reads_nothing_back(case):
    align = torch.from_numpy(AR.random_alignments(3, 300, 40, np.float32, 8)).to(DEV)
    in_d, out_d = torch.tensor([40, 17, 33]).to(DEV), torch.tensor([300, 256, 1]).to(DEV)          # int64, as inference_batch's
    check = AL.AlignmentCheck(skip_max=1, stall_max=2, min_focus=0.5)
    want = [AL.alignment_report(align, in_d, out_d, check), AL.alignment_report(align, [40, 17, 33], [300, 256, 1], check)]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = [AL.alignment_report(align, in_d, out_d, check), AL.alignment_report(align, [40, 17, 33], [300, 256, 1], check)]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    ref = AR.report(align.cpu().numpy(), [40, 17, 33], [300, 256, 1], **thresholds_of(check))
    for g, w in zip(got, want):
        assert all(torch.equal(a, b) for a, b in zip(g, w))
        _same_report(g, ref)


def test_report_on_a_callers_stream():
    """alignment_report on a stream S whose inputs become true only behind a gate on S, a consumer on S"""
    true = torch.from_numpy(AR.random_alignments(4, 500, 64, np.float32, 21)).to(DEV)
    decoy = torch.from_numpy(AR.random_alignments(4, 500, 64, np.float32, 22)).to(DEV)
    true_l, decoy_l = torch.tensor([500, 300, 77, 1], dtype=torch.int32).to(DEV), torch.tensor([9, 500, 2, 400], dtype=torch.int32).to(DEV)
    buf, buf_l = decoy.clone(), decoy_l.clone()
    check = AL.AlignmentCheck(skip_max=1, stall_max=2, min_focus=0.5)

    def call():
        return AL.alignment_report(buf, [64, 50, 64, 3], buf_l, check)

    def same(a, b):
        return all(torch.equal(x, y) for x, y in zip(a, b))

    def fill(a, l):
        buf.copy_(a, non_blocking=True)
        buf_l.copy_(l, non_blocking=True)
    fill(true, true_l)
    call()
    ref, ms = SU.timed(lambda: [x.clone() for x in call()])
    fill(decoy, decoy_l)
    dec = [x.clone() for x in call()]
    torch.cuda.synchronize()
    assert not same(dec, ref), "the decoy input gives the true result - the test could not fail"
    n = SU.gate_matmuls(ms)
    SU.log("alignment_report, device lengths", ms, n)
    S = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(S):
        call()
    S.synchronize()
    gate = SU.behind_gate(S, [buf, buf_l], [true, true_l], n)
    with torch.cuda.stream(S):
        out = call()
        gate.check()
        got = [x.clone() for x in out]
    S.synchronize()
    assert same(got, ref), "alignment_report on a caller's stream differs from the default-stream run"
    again = [x.clone() for x in call()]
    torch.cuda.synchronize()
    assert same(again, ref)


def test_checked_long_form_is_its_parts_and_its_solo_chains(case):
    t, w, check, n = case["t"], case["w"], case["check"], 5
    got = _long(case, check=check, max_attempts=ATTEMPTS)
    assert isinstance(got, L.LongFormChecked)
    # the replay: pass by pass, the documented groups, the verdicts of the restatement on inference_batch's alignments
    n_ids = [i.size(1) for i in case["ids"]]
    pending, attempts, row_of = list(range(n)), [None] * n, {}
    batches, kept_reports, kept_frames, worst_gap = [], [], [], 0.0
    for k in range(ATTEMPTS):
        again = []
        for group, group_seeds in L.plan_pass(n_ids, case["seeds"], pending, k, 2, True):
            assert group_seeds == [case["table"][k][c] for c in group]
            out, rep = _decode_group(case, group, group_seeds)
            flags = rep.flags.tolist()
            for b, c in enumerate(group):
                gap = abs(value(rep, b, case["statistic"]) - value(case["solo"][k][c], 0, case["statistic"]))
                worst_gap = max(worst_gap, gap)
                print("align-check pass %d chunk %d: %s %r in its group, %r alone (differ by %.3g), flags %d"
                      % (k, c, case["statistic"], value(rep, b, case["statistic"]), value(case["solo"][k][c], 0, case["statistic"]),
                         gap, flags[b]))
            assert flags == [case["predicted"][k][c] for c in group], "a verdict in the group differs from the solo statistic's"
            rows = [b for b, f in enumerate(flags) if f == 0 or k == ATTEMPTS - 1]
            again += [c for b, c in enumerate(group) if b not in rows]
            if not rows:
                continue
            for b in rows:
                attempts[group[b]], row_of[group[b]] = k, len(row_of)
            frames = out[4].cpu()[rows]
            idx = torch.tensor(rows).to(DEV)
            mel = out[1] if len(rows) == len(group) else out[1][:, :, :int(frames.max())].index_select(0, idx)
            batches.append(w.infer_batch(mel, frames, sigma=U.SIGMA, seeds=[group_seeds[b] for b in rows]))
            kept_reports.append((rep, rows))
            kept_frames += frames.tolist()
        pending = sorted(again)
        if not pending:
            break
    print("align-check: attempts %s, margin %g, largest batch-to-solo difference of %s %.3g"
          % (attempts, case["margin"], case["statistic"], worst_gap))
    assert worst_gap <= case["margin"], "the margin is smaller than the measured batch-to-solo difference"
    assert 0 in attempts and max(attempts) > 0, "no chunk passed at once, or none went again: the test shows nothing"
    order = [row_of[p] for p in range(n)]
    pause = L.ms_to_samples(PAUSE_MS, RATE)
    audio, length, offsets = A.join_batches(batches, order=order, pause=pause, fade=0)
    assert got.attempts.dtype == torch.int64 and got.attempts.tolist() == attempts
    assert torch.equal(got.audio, audio) and torch.equal(got.length, length) and torch.equal(got.offsets, offsets)
    # the report of the attempt kept, in the text's order
    want_rows = {}
    for rep, rows in kept_reports:
        for b in rows:
            want_rows[len(want_rows)] = (rep, b)
    by_chunk = [want_rows[order[p]] for p in range(n)]
    assert got.flags.cpu().tolist() == [int(rep.flags[b]) for rep, b in by_chunk]
    assert got.flags.cpu().tolist() == [case["predicted"][attempts[c]][c] for c in range(n)]
    assert got.stats.cpu().tolist() == [rep.stats[b].tolist() for rep, b in by_chunk]
    assert tuple(got.durations.shape) == (n, max(n_ids))
    for c, (rep, b) in enumerate(by_chunk):
        d = rep.dur[b].tolist()
        assert got.durations[c].cpu().tolist() == d + [0] * (max(n_ids) - len(d))
        assert abs(float(got.focus[c]) - rep.focus[b]) <= AR.focus_bound(rep.peak[b], int(rep.stats[b, 0]))
    assert got.truncated.tolist() == [kept_frames[order[p]] == U.N_STEPS for p in range(n)] and got.chunks == U.CHUNKS
    # every chunk against its solo chain under the seed of the attempt it is spoken with
    off = got.offsets.cpu().tolist()
    a = got.audio[0].cpu().numpy()
    worst = 0.0
    for c in range(n):
        s = case["table"][attempts[c]][c]
        solo = w.infer(case["solo_mel"][attempts[c]][c], sigma=U.SIGMA, seed=s)[0].cpu().numpy()
        assert off[c + 1] - off[c] - (pause if c < n - 1 else 0) == solo.size, "chunk %d's length differs from its solo chain's" % c
        e = R.rel(a[off[c]:off[c] + solo.size], solo)
        worst = max(worst, e)
        print("align-check chunk %d, attempt %d (%d samples) vs its solo chain: rel %.2e" % (c, attempts[c], solo.size, e))
    assert worst < SOLO_BAR
    # ... whatever the grouping
    for bs, sort in ((5, False), (1, True)):
        other = _long(case, check=check, max_attempts=ATTEMPTS, batch_size=bs, sort_by_length=sort)
        assert other.attempts.tolist() == attempts and torch.equal(other.offsets, got.offsets)
        assert other.flags.tolist() == got.flags.tolist() and other.stats[:, :2].tolist() == got.stats[:, :2].tolist()
        e = R.rel(other.audio[0, :off[n]], got.audio[0, :off[n]])
        print("align-check batch_size %d sort %s vs batch_size 2: rel %.2e" % (bs, sort, e))
        assert e < SOLO_BAR


def test_one_attempt_is_the_unchecked_call_with_flags(case):
    plain = _long(case)
    assert type(plain) is L.LongForm and len(plain) == 5
    got = _long(case, check=case["check"], max_attempts=1)
    assert isinstance(got, L.LongFormChecked)
    assert all(torch.equal(x, y) for x, y in zip(got[:3], plain[:3])) and torch.equal(got.truncated, plain.truncated)
    assert got.chunks == plain.chunks and got.attempts.tolist() == [0] * 5
    assert got.flags.cpu().tolist() == case["predicted"][0] and any(got.flags.cpu().tolist())
    again = _long(case, check=None, max_attempts=1)
    assert type(again) is L.LongForm and torch.equal(again.audio, plain.audio)
