"""Long-form synthesis: a paragraph as one utterance in HBM.

The decoder stops at max_decoder_steps frames (1000: 5.7 s at hop 256 and 44 800 Hz), so a text longer than a sentence or two is
split into chunks (``split_text``), the chunks are decoded and vocoded in ragged batches (``Tacotron.inference_batch(seeds=)``,
``WaveGlow.infer_batch(seeds=)``, optionally ``Denoiser.denoise_batch`` and ``Trimmer.trim_batch``), and the rows of those batches
are joined - sentence after sentence, a pause between them, a short ramp at every joint - by ``audio.join_batches``
(csrc/join.hip), optionally resampled and quantised.  Every chunk has a seed of its own (``chunk_seeds``), so its audio is a
function of (seed, its index, its text) and not of the batch it was computed in.  ``synthesize_long`` is the chain; with
``check=`` it looks at every chunk's attention path first (``alignment.alignment_report``) and, with ``max_attempts`` > 1, decodes a
flagged chunk again under another seed (``plan_pass`` / ``settle_pass`` / ``plan_retries`` are the host planning).
``synthesize_long_timed`` is the same chain with a speaking rate and the time of every symbol (``rate.warp_mel``,
``rate.symbol_spans``)."""
import collections

import torch

from . import _lib, sampling
from .text import text_to_sequence

SAMPLING_RATE = 44800          # the project's rate (the reference's hparams.py); synthesize_long(sampling_rate=) overrides it
MAX_SYMBOLS = 64               # split_text's default: a guess, see there
PAUSE_MS, FADE_MS = 250.0, 5.0

_MASK = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15
SENTENCE_END = ".?!。．？！"               # . ? ! and the full-width 。 ． ？ ！
CLAUSE_END = ",;:，；：、"                 # , ; : and the full-width ， ； ： 、

LongForm = collections.namedtuple("LongForm", "audio length offsets chunks truncated")
LongFormChecked = collections.namedtuple("LongFormChecked", LongForm._fields + ("flags", "attempts", "stats", "focus", "durations"))
# ... and with timestamps=True: the same fields, then spans
LongFormTimed = collections.namedtuple("LongFormTimed", LongForm._fields + ("spans",))
LongFormCheckedTimed = collections.namedtuple("LongFormCheckedTimed", LongFormChecked._fields + ("spans",))


def mix(x):
    """splitmix64's finaliser on a wrapping uint64, as include/t2s_hip.h states it for the keyed draws"""
    x &= _MASK
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & _MASK
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & _MASK
    x ^= x >> 31
    return x


def chunk_seeds(seed, n):
    """One seed per chunk from the utterance's: s_i = mix((i + 1) GOLD + seed) >> 1 in wrapping uint64 arithmetic, n Python ints in
    [0, 2^63).  Chunk i's draws then depend on (seed, i) alone - not on the batch size or on the order the chunks were grouped in."""
    seed = sampling.check_seed(seed, "chunk_seeds: seed")
    n = int(n)
    if n < 0:
        raise ValueError("chunk_seeds: n must be >= 0, got %d" % n)
    return [mix((i + 1) * GOLD + seed) >> 1 for i in range(n)]


def n_symbols(text):
    """ids the text becomes, the end-of-sequence id included: what the encoder sees"""
    return len(text_to_sequence(text))


def _pack(tokens, max_symbols):
    """Consecutive tokens joined by single spaces into as few pieces of at most max_symbols ids as a left-to-right pass gives;
    a token that is too long alone is returned alone (the caller cuts it further or refuses it)."""
    pieces, cur = [], None
    for t in tokens:
        cand = t if cur is None else cur + " " + t
        if cur is None or n_symbols(cand) <= max_symbols:
            cur = cand
        else:
            pieces.append(cur)
            cur = t
    if cur is not None:
        pieces.append(cur)
    return pieces


def _runs(words, marks):
    """the words grouped into runs that end behind a word whose last character is one of `marks` (it stays with the left part)"""
    runs, cur = [], []
    for w in words:
        cur.append(w)
        if w[-1] in marks:
            runs.append(" ".join(cur))
            cur = []
    if cur:
        runs.append(" ".join(cur))
    return runs


def split_text(text, max_symbols=MAX_SYMBOLS):
    """A text as a list of chunks for ``synthesize_long``; host only.  It is cut behind ``. ? !`` and their full-width forms where
    whitespace or the end follows: one sentence, one chunk.  A sentence of more than ``max_symbols`` ids
    (``len(text_to_sequence(s))``, the end-of-sequence id included) is cut further behind ``, ; :`` (and their full-width forms), and
    a clause that is still too long at whitespace; neighbouring parts of a sentence are put together again, left to right, as long
    as they fit.  The punctuation stays with the part on its left.  A word that exceeds max_symbols alone raises ValueError; empty
    pieces are dropped.  ``" ".join(split_text(t)) == " ".join(t.split())``: nothing but whitespace is lost.

    The default max_symbols = 64 is a guess at what a decoder trained on sentence-length clips speaks inside its 1000 frames (about
    14 jamo a second for 5.7 s, with room to spare); no trained checkpoint has been measured here.  A chunk that does run into
    max_decoder_steps is reported by synthesize_long's ``truncated``."""
    if not isinstance(text, str):
        raise ValueError("split_text: text must be a str, got %s" % type(text).__name__)
    max_symbols = int(max_symbols)
    if max_symbols < 2:
        raise ValueError("split_text: max_symbols must be at least 2 (one symbol and the end-of-sequence id), got %d" % max_symbols)
    chunks = []
    for sentence in _runs(text.split(), SENTENCE_END):
        if n_symbols(sentence) <= max_symbols:
            chunks.append(sentence)
            continue
        parts = []
        for clause in _runs(sentence.split(" "), CLAUSE_END):
            if n_symbols(clause) <= max_symbols:
                parts.append(clause)
                continue
            for piece in _pack(clause.split(" "), max_symbols):
                if n_symbols(piece) > max_symbols:
                    raise ValueError("split_text: %r is %d symbols without whitespace to cut at, max_symbols is %d"
                                     % (piece, n_symbols(piece), max_symbols))
                parts.append(piece)
        chunks += _pack(parts, max_symbols)
    return chunks


def ms_to_samples(ms, rate, what="ms_to_samples"):
    """round(ms rate / 1000) as a host int; a negative or non-finite duration raises ValueError"""
    try:
        v = float(ms) * rate / 1000.0
    except (TypeError, ValueError):
        raise ValueError("%s: a duration in milliseconds must be a number, got %r" % (what, ms)) from None
    if not (v >= 0.0 and v - v == 0.0):
        raise ValueError("%s: a duration must be finite and not negative, got %r ms" % (what, ms))
    return int(round(v))


def _plan(n_ids, batch_size, sort_by_length):
    """(groups of chunk indices, order: position -> row of the join) - rows are numbered through the groups"""
    idx = list(range(len(n_ids)))
    if sort_by_length:
        idx.sort(key=lambda i: -n_ids[i])                       # (stable: equal counts keep their order)
    groups = [idx[g:g + batch_size] for g in range(0, len(idx), batch_size)]
    row_of = {c: r for r, c in enumerate(idx)}
    return groups, [row_of[p] for p in range(len(idx))]


def plan_pass(n_ids, seeds, pending, k, batch_size, sort_by_length):
    """Pass k of synthesize_long(check=) over the chunks `pending` (chunk indices, ascending): they are grouped by ``_plan`` as a text
    of their own would be -> [(the group's chunks, their seeds ``attempt_seeds(seeds[c], k)``)].  Host only."""
    from .alignment import attempt_seeds
    groups, _ = _plan([n_ids[c] for c in pending], batch_size, sort_by_length)
    return [([pending[i] for i in g], [attempt_seeds(seeds[pending[i]], k) for i in g]) for g in groups]


def settle_pass(flags, k, max_attempts):
    """The rows of a group that are kept at attempt k, given their flags: those with flags 0, and every row at the last attempt"""
    return [b for b, f in enumerate(flags) if f == 0 or k >= max_attempts - 1]


def _run_passes(n_ids, seeds, batch_size, sort_by_length, max_attempts, decode, keep):
    """The retry loop.  ``decode(k, chunks, seeds) -> (flags, handle)`` decodes one group and reports one int of flags per row;
    ``keep(handle, rows, chunks, seeds)`` speaks the kept rows.  Kept rows are numbered through the passes and groups in the order
    they are kept -> (passes: per pass a list of (chunks, seeds, kept rows), attempts per chunk, order: position -> row)."""
    n = len(n_ids)
    pending, attempts, row_of, passes = list(range(n)), [0] * n, {}, []
    for k in range(max_attempts):
        if not pending:
            break
        this, again = [], []
        for chunks, s in plan_pass(n_ids, seeds, pending, k, batch_size, sort_by_length):
            flags, handle = decode(k, chunks, s)
            kept = settle_pass(flags, k, max_attempts)
            for b in kept:
                attempts[chunks[b]] = k
                row_of[chunks[b]] = len(row_of)
            again += [c for b, c in enumerate(chunks) if b not in kept]
            if kept:
                keep(handle, kept, chunks, s)
            this.append((chunks, s, kept))
        passes.append(this)
        pending = sorted(again)
    return passes, attempts, [row_of[p] for p in range(n)]


def plan_retries(n_ids, seeds, flag_table, batch_size=8, sort_by_length=True, max_attempts=1):
    """What synthesize_long(check=, max_attempts=) does, given the flags beforehand: ``flag_table[k][i]`` are the flags chunk i gets
    at attempt k (0: it passes).  Chunk i is spoken with its first attempt that passes, or else with its last.  Returns (passes,
    attempts, order): per pass the list of its groups as (chunks, seeds, rows of the group that are kept); the attempt every chunk is
    spoken with; and position -> row of the join, the kept rows numbered through the passes and groups.  Host only."""
    return _run_passes(n_ids, seeds, int(batch_size), sort_by_length, int(max_attempts),
                       lambda k, chunks, s: ([flag_table[k][c] for c in chunks], None), lambda *a: None)


def _check_long_args(tacotron, waveglow, text, chunks, seed, seeds, batch_size, max_symbols, pause_ms, pauses_ms, fade_ms, rate):
    """Every check of synthesize_long that needs no device -> (chunks, ids per chunk, seeds, pauses in samples, fade in samples)"""
    who = "synthesize_long"
    T2SError = _lib.T2SError
    if tacotron.training or waveglow.training:
        raise T2SError("%s runs in eval mode only (call .eval() on both models)" % who)
    if (text is None) == (chunks is None):
        raise T2SError("%s: give text or chunks, exactly one" % who)
    if (seed is None) == (seeds is None):
        raise T2SError("%s: a seed is required, seed or seeds (one per chunk) - without one a chunk's draws depend on its batch"
                       % who)
    if int(batch_size) != batch_size or batch_size < 1:
        raise ValueError("%s: batch_size must be an integer >= 1, got %r" % (who, batch_size))
    if int(rate) != rate or rate < 1:
        raise ValueError("%s: sampling_rate must be a positive integer, got %r" % (who, rate))
    if text is not None:
        chunks = split_text(text, max_symbols)
    else:
        if isinstance(chunks, str):
            raise T2SError("%s: chunks must be a sequence of strings, not one string (that is text=)" % who)
        chunks = list(chunks)
        if not all(isinstance(c, str) for c in chunks):
            raise T2SError("%s: chunks must be strings" % who)
    if not chunks:
        raise T2SError("%s: nothing to say - the text holds no chunk" % who)
    n = len(chunks)
    if n > 65535:
        raise T2SError("%s: %d chunks, the most is 65535" % (who, n))
    ids = [text_to_sequence(c) for c in chunks]
    if seeds is None:
        seeds = chunk_seeds(seed, n)
    else:
        try:
            seeds = [sampling.check_seed(s, "%s: seeds" % who) for s in seeds]
        except TypeError:
            raise ValueError("%s: seeds must be a sequence of integers" % who) from None
        if len(seeds) != n:
            raise ValueError("%s: seeds holds %d values, there are %d chunks" % (who, len(seeds), n))
    if pauses_ms is not None:
        try:
            gaps = [ms_to_samples(ms, rate, who) for ms in pauses_ms]
        except TypeError:
            raise ValueError("%s: pauses_ms must be a sequence of numbers" % who) from None
        if len(gaps) != n - 1:
            raise ValueError("%s: pauses_ms holds %d values, %d chunks need %d" % (who, len(gaps), n, n - 1))
    else:
        gaps = [ms_to_samples(pause_ms, rate, who)] * (n - 1)
    return chunks, ids, seeds, gaps, ms_to_samples(fade_ms, rate, who)


def synthesize_long(tacotron, waveglow, text=None, *, chunks=None, seed=None, seeds=None, sigma=0.666, batch_size=8,
                    max_symbols=MAX_SYMBOLS, sort_by_length=True, denoiser=None, strength=0.1, trimmer=None, pause_ms=PAUSE_MS,
                    pauses_ms=None, fade_ms=FADE_MS, resampler=None, pcm16=False, sampling_rate=None, check=None, max_attempts=1):
    """Text of any length -> one utterance in HBM.  ``text`` is split by ``split_text(text, max_symbols)``, or ``chunks`` (strings)
    are taken as they are; each goes through ``text_to_sequence``.  Groups of ``batch_size`` chunks (8 is the largest batch on the
    fp16 decode path) run ``tacotron.inference_batch(seeds=)`` -> ``waveglow.infer_batch(sigma, seeds=)`` -> ``denoiser.denoise_batch
    (strength)`` and ``trimmer.trim_batch`` where given; with ``sort_by_length`` the groups are taken in order of decreasing id
    count, so that chunks of similar length share a batch (both models also compute their padding).  One ``audio.join_batches`` over
    all groups puts the chunks back in the text's order with ``pause_ms`` of silence between them (``pauses_ms``: one value per
    joint) and ``fade_ms`` of ramp at every joint; then ``resampler.resample_batch`` and ``audio.to_pcm16`` where asked.
    Milliseconds become samples at the vocoder's rate, round(ms rate / 1000) on the host; the rate is ``sampling_rate``, else the
    resampler's orig_rate, else 44 800.

    A seed is required: ``seed`` (chunk i gets ``chunk_seeds(seed, n)[i]`` for both its prenet masks and its vocoder noise) or
    ``seeds``, one int in [0, 2^63) per chunk.  Chunk i's samples are then those of
    ``infer(inference(ids_i, seed=s_i).mel_post, sigma, seed=s_i)`` up to float rounding, whatever batch_size and sort_by_length.
    Eval mode only.

    Returns LongForm(audio, length, offsets, chunks, truncated):
      audio      [1, cap] float32 (int16 with pcm16), zeros behind ``length``
      length     [1] on the device: the utterance's samples, at the output rate
      offsets    int64 [n + 1] on the device: chunk i starts at offsets[i] and the joined samples end at offsets[n] - in samples
                 at the VOCODER's rate, before any resampling
      chunks     the chunk strings
      truncated  bool [n] on the device: chunk i ran into max_decoder_steps without a stop (its audio is cut there; split finer)

    The host reads one thing per group from the device: the output lengths, once, directly behind ``inference_batch`` (whose
    decode loop polls the device anyway) - ``infer_batch`` and ``denoise_batch`` size their launches by them.  Behind that read
    nothing in the group's chain, in the join or in the resampling reads the device; the lengths the trimmer finds never leave it.

    ``check`` (an ``alignment.AlignmentCheck``) looks at every chunk's attention path before it is spoken, and ``max_attempts`` > 1
    decodes a flagged chunk again.  Pass k = 0, 1, ... takes the chunks not yet accepted, groups them as above (``plan_pass``),
    decodes each group with ``inference_batch(seeds=attempt_seeds(s_i, k))`` and runs ``alignment.alignment_report`` on the
    alignments; the group's one read-back then brings the flags along with the output lengths (one stacked tensor, one copy).  A
    chunk whose flags are 0 is accepted, and at pass max_attempts - 1 every remaining one is: chunk i is spoken with its first
    attempt that passes, or else with its last, through ``infer_batch -> denoise_batch -> trim_batch`` under the same attempt seed -
    the audio of its solo chain under ``attempt_seeds(s_i, a_i)`` up to float rounding, whatever batch_size and sort_by_length.
    A group with a rejected row pays one index copy of its accepted rows' mel before the vocoder
    (``mel_post[:, :, :N'].index_select(0, rows)``, N' their longest) and small ones of their lengths, seeds and report; a group
    without one pays nothing.  The join takes the accepted rows of all passes through ``order``.  A check's ``max_frames=None``
    is the decoder's max_decoder_steps.  The result is then LongFormChecked: LongForm's five fields (``truncated`` as before, of the
    attempt kept), and
      flags      int32 [n] on the device: the kept attempt's flags (0: it passed; alignment.FLAG_NAMES)
      attempts   int64 [n] on the host: the attempt chunk i is spoken with
      stats      int32 [n, 8], focus float64 [n], durations int32 [n, longest chunk's ids] on the device: the kept attempt's
                 report in the text's order (durations: frames per symbol, before trimming and resampling)
    ``check=None`` with ``max_attempts=1`` is the call without either: the same launches, a LongForm.

    ``synthesize_long_timed`` is this call with two more keywords, ``speed`` and ``timestamps``: another speaking rate, and the
    time of every symbol in the audio returned.  The keyword list of this one is pinned by a test, so they live there."""
    return synthesize_long_timed(tacotron, waveglow, text, chunks=chunks, seed=seed, seeds=seeds, sigma=sigma, batch_size=batch_size,
                                 max_symbols=max_symbols, sort_by_length=sort_by_length, denoiser=denoiser, strength=strength,
                                 trimmer=trimmer, pause_ms=pause_ms, pauses_ms=pauses_ms, fade_ms=fade_ms, resampler=resampler,
                                 pcm16=pcm16, sampling_rate=sampling_rate, check=check, max_attempts=max_attempts)


def synthesize_long_timed(tacotron, waveglow, text=None, *, chunks=None, seed=None, seeds=None, sigma=0.666, batch_size=8,
                          max_symbols=MAX_SYMBOLS, sort_by_length=True, denoiser=None, strength=0.1, trimmer=None, pause_ms=PAUSE_MS,
                          pauses_ms=None, fade_ms=FADE_MS, resampler=None, pcm16=False, sampling_rate=None, check=None, max_attempts=1,
                          speed=None, timestamps=False):
    """``synthesize_long`` - every argument, default and result of it, see there - at another speaking rate and with the time of
    every symbol.  Without the two keywords it is that call: the same launches, the same result.

    ``speed`` (a float in [1 / 8, 8], or one per chunk; 2 is twice as fast) changes the speaking rate without touching pitch: every
    group's ``mel_post`` goes through ``rate.warp_mel`` between ``inference_batch`` and ``infer_batch``, and the vocoder makes
    ``rate.warped_length(frames_i, speed_i)`` frames of samples for chunk i - an integer the host forms from the frames the group's
    one read-back already brought, so there is no second one.  Chunk i's samples are then those of
    ``infer(warp_mel(inference(ids_i, seed=s_i).mel_post, None, speed_i).mel, sigma, seed=s_i)`` up to float rounding.  ``speed=1.0``
    gives the audio of ``speed=None`` bit for bit (the warp is the identity); ``speed=None`` issues the launches it always did.
    Per-symbol rates are reachable through ``warp_mel`` only.

    ``timestamps=True`` adds ``spans`` to the result (a LongFormTimed, or a LongFormCheckedTimed with a check): int64
    [n, longest chunk's ids, 2] on the device, in the text's order - symbol k of chunk i sounds in
    ``audio[0, spans[i, k, 0] : spans[i, k, 1]]``, in samples of the audio RETURNED: behind the warp, the trimmer's cut, the join's
    offsets and the resampler's ratio (``rate.symbol_spans`` states each step); (-1, -1) for a symbol no frame attends to and for
    the padding behind a chunk's ids.  It runs ``alignment_report`` for the path where no check does, asks ``trimmer.bounds_batch``
    for the cut points ``trim_batch`` will use (the same input, the same decision: one more energy pass), and without a ``speed``
    runs the warp at rate 1.  Nothing more is read back.  The other fields keep their meaning; ``durations`` stays the frames per
    symbol of the decoded mel."""
    from . import audio as A
    rate = sampling_rate if sampling_rate is not None else (resampler.orig_rate if resampler is not None else SAMPLING_RATE)
    chunks, ids, seeds, gaps, fade = _check_long_args(tacotron, waveglow, text, chunks, seed, seeds, batch_size, max_symbols, pause_ms,
                                                      pauses_ms, fade_ms, rate)
    if isinstance(max_attempts, bool) or not isinstance(max_attempts, int) or max_attempts < 1:
        raise ValueError("synthesize_long: max_attempts must be an integer >= 1, got %r" % (max_attempts,))
    speeds = _check_speed(speed, len(chunks))
    timing = _Timing(waveglow, trimmer, resampler) if timestamps else None
    if speeds is None and timestamps:
        speeds = [1.0] * len(chunks)
    if check is not None:
        from .alignment import AlignmentCheck
        if not isinstance(check, AlignmentCheck):
            raise _lib.T2SError("synthesize_long: check must be an alignment.AlignmentCheck, got a %s" % type(check).__name__)
        return _synthesize_checked(tacotron, waveglow, chunks, ids, seeds, gaps, fade, sigma, int(batch_size), sort_by_length, denoiser,
                                   strength, trimmer, resampler, pcm16, check, max_attempts, speeds, timing)
    if max_attempts != 1:
        raise ValueError("synthesize_long: max_attempts = %d needs a check to decide who goes again" % max_attempts)
    n = len(chunks)
    n_ids = [len(s) for s in ids]
    groups, order = _plan(n_ids, int(batch_size), sort_by_length)
    dev = next(waveglow.parameters()).device
    stride = int(waveglow.upsample.stride[0])
    T_cap = int(tacotron.decoder.max_decoder_steps)
    rows = [c for g in groups for c in g]                       # row -> chunk
    seeds_d = A._to_device(torch.tensor([seeds[c] for c in rows], dtype=torch.int64), dev)
    batches, flags, r0 = [], [], 0
    for g in groups:
        B, T = len(g), max(n_ids[c] for c in g)
        padded = torch.zeros(B, T, dtype=torch.int64)
        for b, c in enumerate(g):
            padded[b, :n_ids[c]] = torch.from_numpy(ids[c]).to(torch.int64)
        s_d = seeds_d[r0:r0 + B]
        r0 += B
        in_lens = torch.tensor([n_ids[c] for c in g])
        out = tacotron.inference_batch(A._to_device(padded, dev), in_lens, seeds=s_d)
        path = None
        if timing is not None:
            from .alignment import alignment_report
            path = alignment_report(out[3], in_lens, out[4]).path
        frames = out[4].cpu()                                   # the group's one read-back
        flags.append(out[4] == T_cap)
        mel, src_frames, warped = out[1], frames, None
        if speeds is not None:                                  # (frames: from here on the vocoder's, the warped ones)
            from .rate import warp_mel
            warped = warp_mel(mel, src_frames, [speeds[c] for c in g], path=path, input_lengths=in_lens, n_symbols=T)
            mel, frames = warped.mel, warped.host_lengths
        wav, wav_lens = waveglow.infer_batch(mel, frames, sigma=sigma, seeds=s_d)
        if denoiser is not None:
            wav, wav_lens = denoiser.denoise_batch(wav, frames * stride, strength)
        if timing is not None:
            timing.add(warped, in_lens, src_frames, wav, wav_lens)
        if trimmer is not None:
            wav, wav_lens = trimmer.trim_batch(wav, wav_lens)
        batches.append((wav, wav_lens))
    audio, length, offsets = A.join_batches(batches, order=order, pauses=gaps, fade=fade)
    order_d = A._to_device(torch.tensor(order, dtype=torch.int64), dev)
    truncated = torch.cat(flags)[order_d]
    if resampler is not None:
        audio, length = resampler.resample_batch(audio, length)
    if pcm16:
        audio = A.to_pcm16(audio)                               # (zeros behind `length` already)
    if timing is not None:
        return LongFormTimed(audio, length, offsets, chunks, truncated, timing.spans(order, order_d, offsets, length, max(n_ids)))
    return LongForm(audio, length, offsets, chunks, truncated)


def normalize_long(result, loudness):
    """A ``LongForm`` / ``LongFormChecked`` / ``LongFormTimed`` / ``LongFormCheckedTimed`` with its whole utterance brought to
    ``loudness``'s target (``audio.Loudness.normalize_batch`` over ``result.audio`` and ``result.length``): the same tuple with
    ``audio`` replaced.  One gain for the utterance moves no sample in time, so ``length``, ``offsets``, ``spans`` and every other
    field are the objects given.  Nothing is read back.  An int16 result is refused: level first, quantise afterwards."""
    if not isinstance(result, (LongForm, LongFormChecked, LongFormTimed, LongFormCheckedTimed)):
        raise _lib.T2SError("normalize_long: expected a LongForm result of synthesize_long, got a %s" % type(result).__name__)
    if not torch.is_tensor(result.audio) or result.audio.dtype != torch.float32:
        raise _lib.T2SError("normalize_long: the audio is %s; synthesize with pcm16=False, normalize, then audio.to_pcm16"
                            % getattr(result.audio, "dtype", type(result.audio).__name__))
    audio, _ = loudness.normalize_batch(result.audio, result.length)
    return result._replace(audio=audio)


def limit_long(result, limiter, loudness=None):
    """A ``LongForm`` / ``LongFormChecked`` / ``LongFormTimed`` / ``LongFormCheckedTimed`` with its whole utterance through
    ``limiter`` (``audio.Limiter.limit_batch`` over ``result.audio`` and ``result.length``; with ``loudness``, an
    ``audio.Loudness``, ``normalize_limit_batch``: brought to the target first, in the same pass): the same tuple with ``audio``
    replaced.  A limiter moves no sample in time, so ``length``, ``offsets``, ``spans`` and every other field are the objects
    given.  Nothing is read back.  An int16 result is refused: limit first, quantise afterwards."""
    if not isinstance(result, (LongForm, LongFormChecked, LongFormTimed, LongFormCheckedTimed)):
        raise _lib.T2SError("limit_long: expected a LongForm result of synthesize_long, got a %s" % type(result).__name__)
    if not torch.is_tensor(result.audio) or result.audio.dtype != torch.float32:
        raise _lib.T2SError("limit_long: the audio is %s; synthesize with pcm16=False, limit, then audio.to_pcm16"
                            % getattr(result.audio, "dtype", type(result.audio).__name__))
    if loudness is None:
        audio, _ = limiter.limit_batch(result.audio, result.length)
    else:
        audio, _ = loudness.normalize_limit_batch(result.audio, result.length, limiter)
    return result._replace(audio=audio)


def filter_long(result, filt):
    """A ``LongForm`` / ``LongFormChecked`` / ``LongFormTimed`` / ``LongFormCheckedTimed`` with its whole utterance through ``filt``
    (``audio.SosFilter.filter_batch`` over ``result.audio`` and ``result.length``): the same tuple with ``audio`` replaced.  A
    causal filter stores output i at index i, so ``length``, ``offsets``, ``spans`` and every other field are the objects given -
    but it does delay what it passes: its group delay is NOT compensated, and a span marks where a symbol's samples went in, not
    where the filter's response to them peaks.  Nothing is read back.  An int16 result is refused: filter first, quantise
    afterwards."""
    from .audio import SosFilter
    if not isinstance(result, (LongForm, LongFormChecked, LongFormTimed, LongFormCheckedTimed)):
        raise _lib.T2SError("filter_long: expected a LongForm result of synthesize_long, got a %s" % type(result).__name__)
    if not isinstance(filt, SosFilter):
        raise _lib.T2SError("filter_long: filt must be an audio.SosFilter, got a %s" % type(filt).__name__)
    if not torch.is_tensor(result.audio) or result.audio.dtype != torch.float32:
        raise _lib.T2SError("filter_long: the audio is %s; synthesize with pcm16=False, filter, then audio.to_pcm16"
                            % getattr(result.audio, "dtype", type(result.audio).__name__))
    audio, _ = filt.filter_batch(result.audio, result.length)
    return result._replace(audio=audio)


def _check_speed(speed, n):
    """synthesize_long_timed's ``speed`` -> None, or one rate per chunk (each checked by ``rate.stretch_q``)"""
    if speed is None:
        return None
    from .rate import stretch_q
    if isinstance(speed, (list, tuple)):
        if len(speed) != n:
            raise ValueError("synthesize_long_timed: speed holds %d values, there are %d chunks" % (len(speed), n))
        speeds = list(speed)
    else:
        speeds = [speed] * n
    for v in speeds:
        stretch_q(v)
    return [float(v) for v in speeds]


class _Timing:
    """What synthesize_long_timed(timestamps=True) keeps of every spoken group, and the spans it makes of that behind the join."""

    def __init__(self, waveglow, trimmer, resampler):
        self.hop = int(waveglow.upsample.stride[0])
        self.trimmer = trimmer
        self.ratio = (1, 1) if resampler is None else (resampler.up, resampler.down)
        self.groups = []

    def add(self, warped, in_lens, src_frames, wav, wav_lens):
        """behind the denoiser, in front of the trimmer: its cut points are found here, on what trim_batch will see.  Without a
        trimmer the cut is (0, the samples made): a chunk's last span then ends with its audio, not in the pause behind it (the
        warped length is rounded to whole frames, the map is not)"""
        if self.trimmer is None:
            made = wav_lens.to(torch.int64)
            bounds = (torch.zeros_like(made), made)
        else:
            bounds = self.trimmer.bounds_batch(wav, wav_lens)
        self.groups.append((warped, in_lens, src_frames, bounds))

    def spans(self, order, order_d, offsets, length, T_max):
        """int64 [n, T_max, 2] in the text's order; rows are numbered through the groups as the join numbers them"""
        from . import audio as A
        from .rate import symbol_spans
        n = len(order)
        dev = offsets.device
        pos = [0] * n
        for p, r in enumerate(order):
            pos[r] = p
        by_row = offsets.index_select(0, A._to_device(torch.tensor(pos, dtype=torch.int64), dev))
        out = torch.full((n, T_max, 2), -1, dtype=torch.int64, device=dev)
        r0 = 0
        for warped, in_lens, src_frames, bounds in self.groups:
            B = in_lens.numel()
            sp = symbol_spans(warped, None, in_lens, src_frames, self.hop, trim_bounds=bounds, offsets=by_row[r0:r0 + B],
                              ratio=self.ratio, total=length)
            out[r0:r0 + B, :sp.size(1)] = sp
            r0 += B
        return out[order_d]


def _synthesize_checked(tacotron, waveglow, chunks, ids, seeds, gaps, fade, sigma, batch_size, sort_by_length, denoiser, strength,
                        trimmer, resampler, pcm16, check, max_attempts, speeds=None, timing=None):
    """synthesize_long with a check: the passes of ``_run_passes``, each group decoded, reported, read once and its kept rows spoken"""
    from . import audio as A
    from .alignment import alignment_report
    n = len(chunks)
    n_ids = [len(s) for s in ids]
    dev = next(waveglow.parameters()).device
    stride = int(waveglow.upsample.stride[0])
    T_cap = int(tacotron.decoder.max_decoder_steps)
    check = check.with_max_frames(T_cap)
    batches, kept_reports = [], []

    def decode(k, group, group_seeds):
        B, T = len(group), max(n_ids[c] for c in group)
        padded = torch.zeros(B, T, dtype=torch.int64)
        for b, c in enumerate(group):
            padded[b, :n_ids[c]] = torch.from_numpy(ids[c]).to(torch.int64)
        in_lens = torch.tensor([n_ids[c] for c in group])
        s_d = A._to_device(torch.tensor(group_seeds, dtype=torch.int64), dev)
        out = tacotron.inference_batch(A._to_device(padded, dev), in_lens, seeds=s_d)
        rep = alignment_report(out[3], in_lens, out[4], check)
        both = torch.stack([out[4], rep.flags.to(torch.int64)]).cpu()          # the group's one read-back: lengths and flags
        return both[1].tolist(), (out[1], out[4], both[0], s_d, rep, in_lens)

    def keep(handle, rows, group, group_seeds):
        mel, olen, frames, s_d, rep, in_lens = handle
        fields = (rep.flags, rep.stats, rep.focus, rep.durations)
        path = rep.path
        if len(rows) < len(group):                              # rejected rows leave the batch: index copies, no arithmetic
            idx = A._to_device(torch.tensor(rows, dtype=torch.int64), dev)
            frames = frames[rows]
            mel = mel[:, :, :int(frames.max())].index_select(0, idx)
            olen, s_d = olen.index_select(0, idx), s_d.index_select(0, idx)
            fields = tuple(f.index_select(0, idx) for f in fields)
            if speeds is not None:
                in_lens, path = in_lens[rows], path.index_select(0, idx)
        src_frames, warped = frames, None
        if speeds is not None:                                  # (frames: from here on the vocoder's, the warped ones)
            from .rate import warp_mel
            warped = warp_mel(mel, src_frames, [speeds[group[b]] for b in rows], path=path if timing is not None else None,
                              input_lengths=in_lens, n_symbols=rep.durations.size(1))
            mel, frames = warped.mel, warped.host_lengths
        wav, wav_lens = waveglow.infer_batch(mel, frames, sigma=sigma, seeds=s_d)
        if denoiser is not None:
            wav, wav_lens = denoiser.denoise_batch(wav, frames * stride, strength)
        if timing is not None:
            timing.add(warped, in_lens, src_frames, wav, wav_lens)
        if trimmer is not None:
            wav, wav_lens = trimmer.trim_batch(wav, wav_lens)
        batches.append((wav, wav_lens))
        kept_reports.append((olen == T_cap,) + fields)

    _, attempts, order = _run_passes(n_ids, seeds, batch_size, sort_by_length, max_attempts, decode, keep)
    audio, length, offsets = A.join_batches(batches, order=order, pauses=gaps, fade=fade)
    order_d = A._to_device(torch.tensor(order, dtype=torch.int64), dev)
    truncated, flags, stats, focus = (torch.cat([r[i] for r in kept_reports])[order_d] for i in range(4))
    durations = torch.zeros(n, max(n_ids), dtype=torch.int32, device=dev)
    r0 = 0
    for r in kept_reports:                                      # (a group's durations are as wide as its longest chunk)
        durations[r0:r0 + r[4].size(0), :r[4].size(1)] = r[4]
        r0 += r[4].size(0)
    durations = durations[order_d]
    if resampler is not None:
        audio, length = resampler.resample_batch(audio, length)
    if pcm16:
        audio = A.to_pcm16(audio)
    result = LongFormChecked(audio, length, offsets, chunks, truncated, flags, torch.tensor(attempts, dtype=torch.int64), stats, focus,
                             durations)
    if timing is not None:
        return LongFormCheckedTimed(*result, timing.spans(order, order_d, offsets, length, max(n_ids)))
    return result
