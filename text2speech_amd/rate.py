"""Speaking rate and symbol timestamps: a mel warped in time on the device, and where every symbol lies in the audio.

Tacotron-2 has no duration input, so speed is changed between the two models: ``warp_mel`` stretches the frame axis of ``mel_post``
(csrc/warp.hip; include/t2s_hip.h states the arithmetic) and WaveGlow makes more or fewer samples - pitch and timbre stay, where
stretching the finished audio would smear phases.  The warp is driven by a cumulative map of exact integers (output frames per source
frame in units of 1 / 2^20), and the same map is what ``symbol_spans`` reads timestamps from: [start, end) of every symbol in samples,
optionally carried through a ``Trimmer``'s cut, ``join_batches``' offsets and a ``Resampler``'s ratio.  ``stretch_q`` and
``warped_length`` are the host's side of the definition: a caller who knows the frames and a uniform rate knows the warped length
without a read-back.  ``synthesize_long_timed(speed=, timestamps=)`` is the chain.

``WarpStream`` is the same warp pushed piece by piece (csrc/warp.hip): the cumulative map persists in HBM and is its own carry,
``settled_length`` says which output frames no later frame can change, and the pieces are ``warp_mel``'s frames bit for bit -
``synthesize_stream(control=StreamControl(speed=))`` is that chain.

Not covered: rates that vary inside a symbol, pitch or energy control, per-symbol rate tables inside a stream."""
import collections
import operator

import torch

from . import _lib

__all__ = ["Q", "WarpedMel", "stretch_q", "warped_length", "settled_length", "warp_mel", "symbol_spans", "WarpStream"]

Q = 1 << 20                    # a stretch counts output frames in units of 1 / Q
RATE_LO, RATE_HI = 0.125, 8.0  # the library's limits on a rate (include/t2s_hip.h)
MIN_RATE, MAX_RATE = 0.5, 2.0  # the default clamp of a per-symbol table
NO_TOTAL = 1 << 62

_KINDS = {torch.float32: 1, torch.float16: 2}

WarpedMel = collections.namedtuple("WarpedMel", "mel lengths cum first_last host_lengths")


def stretch_q(rate):
    """rint(Q / rate) in double, ties to even: the output frames every source frame becomes at ``rate``, in units of 1 / Q.
    rate 1 -> Q, 0.5 (half speed) -> 2 Q.  A rate outside [1 / 8, 8], or not a finite number, raises ValueError."""
    try:
        rate = None if isinstance(rate, (bool, str, bytes)) else float(rate)
    except (TypeError, ValueError):
        rate = None
    if rate is None:
        raise ValueError("stretch_q: a rate must be a number")
    if not RATE_LO <= rate <= RATE_HI:                          # (false for a NaN)
        raise ValueError("stretch_q: a rate must lie in [%g, %g], got %r" % (RATE_LO, RATE_HI, rate))
    return round(Q / rate)


def _warped(frames, s, cap=None):
    if frames <= 0:
        return 0
    n = max(1, (frames * s + Q // 2) >> 20)
    return n if cap is None else min(n, cap)


def warped_length(frames, rate, cap=None):
    """The frames ``warp_mel`` makes of ``frames`` source frames at a uniform ``rate``: 0 for 0, else
    max(1, (frames stretch_q(rate) + Q / 2) >> 20), cut to ``cap`` where given - the map kernel's own integer."""
    try:
        frames = None if isinstance(frames, bool) else operator.index(frames)
    except TypeError:
        frames = None
    if frames is None or frames < 0:
        raise ValueError("warped_length: frames must be an integer >= 0")
    return _warped(frames, stretch_q(rate), cap)


def settled_length(cum_before_last, cum_last, final=False):
    """The output frames of a streamed warp that no later source frame can change, over exact Python integers.  With n source frames
    seen, ``cum_before_last`` = c[n - 1] and ``cum_last`` = c[n] of the cumulative map (both 0 for n = 0; c[0] = 0 for n = 1):
    output frame j interpolates between the source frames whose doubled centres m[f] = c[f] + c[f + 1] enclose (2j + 1) Q, so it is
    settled once (2j + 1) Q <= m[n - 1] - the count is #{j >= 0 : (2j + 1) Q <= c[n - 1] + c[n]} = (c[n - 1] + c[n] + Q) // 2Q.
    At rate 1 that is n: no lag.  ``final``: the utterance ends at frame n, and the count is ``warped_length``'s integer, 0 for
    c[n] = 0 and else max(1, (c[n] + Q / 2) >> 20).  The host mirrors c from the stretches it passed (``stretch_q``), so it knows
    every count without a read-back."""
    try:
        a, b = (None if isinstance(v, bool) else operator.index(v) for v in (cum_before_last, cum_last))
    except TypeError:
        a = b = None
    if a is None or b is None or not 0 <= a <= b:
        raise ValueError("settled_length: needs integers 0 <= c[n - 1] <= c[n], got %r and %r" % (cum_before_last, cum_last))
    if final:
        return 0 if b == 0 else max(1, (b + Q // 2) >> 20)
    return 0 if b == 0 else (a + b + Q) // (2 * Q)


def _lengths(lengths, B, hi, dev, who, what):
    """[B] lengths for the kernels -> (int32 on the device or None, host int64 clamped to [0, hi] or None).  A device tensor is used as
    it is (an int64 one through a cast - a copy, its values are not looked at); host values go up through page-locked memory without
    a wait.  None: every entry whole."""
    from .audio import _to_device
    T2SError = _lib.T2SError
    if lengths is None:
        return None, torch.full((B,), hi, dtype=torch.int64)
    try:
        lens = torch.as_tensor(lengths)
    except (TypeError, ValueError, RuntimeError) as e:
        raise T2SError("%s: %s must be a tensor or a sequence of integers (%s)" % (who, what, e))
    if lens.is_floating_point() or lens.is_complex() or lens.dtype == torch.bool:
        raise T2SError("%s: %s must be integers, got %s" % (who, what, lens.dtype))
    if lens.dim() != 1 or lens.numel() != B:
        raise T2SError("%s: %s has shape %s, the batch holds %d entries" % (who, what, tuple(lens.shape), B))
    lens = lens.detach()
    if lens.is_cuda:
        if lens.device != dev:
            raise T2SError("%s: %s live on %s, the data on %s" % (who, what, lens.device, dev))
        return lens.to(torch.int32).contiguous(), None
    host = lens.to(torch.int64).clamp(0, hi)
    return _to_device(host.to(torch.int32), dev), host


def _rows(t, B, width, dtype, dev, who, what):
    """a [B, >= width] device table whose last dimension is dense -> (tensor, elements between rows)"""
    T2SError = _lib.T2SError
    if not (torch.is_tensor(t) and t.is_cuda and t.device == dev):
        raise T2SError("%s: %s must be a tensor on %s" % (who, what, dev))
    if t.dtype != dtype:
        raise T2SError("%s: %s must be %s, got %s" % (who, what, dtype, t.dtype))
    if t.dim() != 2 or t.size(0) != B or t.size(1) < width:
        raise T2SError("%s: %s must be [%d, >= %d], got %s" % (who, what, B, width, tuple(t.shape)))
    t = t.detach()
    if t.stride(1) != 1 or (B > 1 and t.stride(0) < t.size(1)):
        t = t.contiguous()
    return t, (t.stride(0) if B > 1 else t.size(1))


def _stretches(rate, B, who):
    """``rate`` (a number or B of them on the host) -> B stretches"""
    if torch.is_tensor(rate):
        if rate.is_cuda:
            raise _lib.T2SError("%s: rate must be host values (a per-symbol table on the device goes in as symbol_rates)" % who)
        rate = rate.tolist()
    if isinstance(rate, (list, tuple)):
        if len(rate) != B:
            raise ValueError("%s: rate holds %d values, the batch holds %d entries" % (who, len(rate), B))
        return [stretch_q(r) for r in rate]
    return [stretch_q(rate)] * B


def _map(dev, B, F, lens_d, stretches, cap, path=None, ld_path=0, rates=None, ld_rates=0, in_len=None, T_in=0, min_rate=MIN_RATE,
         max_rate=MAX_RATE, want_cum=True):
    """t2s_warp_map -> (cum int64 [B, F + 1] or None, lengths int32 [B], first_last int32 [B, T_in, 2] or None)"""
    from .audio import _to_device
    p = _lib.ptr
    s_d = None
    if len(set(stretches)) > 1:
        s_d = _to_device(torch.tensor(stretches, dtype=torch.int64), dev)
    with torch.cuda.device(dev):
        cum = torch.empty(B, F + 1, dtype=torch.int64, device=dev) if want_cum else None
        out_len = torch.empty(B, dtype=torch.int32, device=dev)
        fl = torch.empty(B, T_in, 2, dtype=torch.int32, device=dev) if path is not None else None
        _lib.call("t2s_warp_map", p(lens_d), B, F, stretches[0], p(s_d), p(path), ld_path, p(rates), ld_rates, p(in_len), T_in,
                  float(min_rate), float(max_rate), cap, p(cum), p(out_len), p(fl), _lib.current_stream())
    return cum, out_len, fl


def _path_args(path, symbol_rates, input_lengths, n_symbols, B, F, dev, who):
    """the checks that a path, a table and the symbols' lengths share -> (path, ld_path, rates, ld_rates, in_len, T_in)"""
    T2SError = _lib.T2SError
    if path is None:
        if symbol_rates is not None:
            raise T2SError("%s: symbol_rates needs path (alignment_report's), the symbol every frame attends to" % who)
        return None, 0, None, 0, None, 0
    path, ld_path = _rows(path, B, F, torch.int32, dev, who, "path")
    rates, ld_rates = None, 0
    if symbol_rates is not None:
        rates, ld_rates = _rows(symbol_rates, B, 1, torch.float32, dev, who, "symbol_rates")
        T_in = rates.size(1)
        if n_symbols is not None and n_symbols != T_in:
            raise T2SError("%s: n_symbols = %d, symbol_rates holds %d columns" % (who, n_symbols, T_in))
    elif n_symbols is not None:
        T_in = operator.index(n_symbols)
    elif input_lengths is not None and not (torch.is_tensor(input_lengths) and input_lengths.is_cuda):
        T_in = int(torch.as_tensor(input_lengths).max())
    else:
        raise T2SError("%s: how many symbols a row holds is not known - give n_symbols (alignments.size(2)), host input_lengths or "
                       "symbol_rates" % who)
    if T_in < 1 or B * T_in > 2 ** 31 - 1:
        raise T2SError("%s: %d entries of %d symbols; one symbol at least, B T_in at most 2^31 - 1" % (who, B, T_in))
    in_len, _ = _lengths(input_lengths, B, T_in, dev, who, "input_lengths")
    return path, ld_path, rates, ld_rates, in_len, T_in


def _clamp_rates(min_rate, max_rate, who):
    try:
        lo, hi = float(min_rate), float(max_rate)
    except (TypeError, ValueError):
        raise ValueError("%s: min_rate and max_rate must be numbers" % who) from None
    if not (RATE_LO <= lo <= hi <= RATE_HI):
        raise ValueError("%s: need %g <= min_rate <= max_rate <= %g, got %r and %r" % (who, RATE_LO, RATE_HI, min_rate, max_rate))
    return lo, hi


def warp_mel(mel, lengths, rate=1.0, *, path=None, symbol_rates=None, input_lengths=None, min_rate=MIN_RATE, max_rate=MAX_RATE,
             cap=None, n_symbols=None):
    """A batch of mels at another speaking rate, computed on the device: rate 2 is twice as fast (half the frames), 0.5 half as fast.

    ``mel`` [B, C, F] float32 or float16 in HBM, e.g. ``inference_batch``'s ``mel_post``; a view whose last dimension is dense and
    whose rows and entries do not overlap (``mel_post[:, :, :N']``) is read where it is, any other is copied first.  ``lengths`` [B]:
    the frames of every entry (None: F).  A device tensor (int32, or int64 as ``inference_batch`` returns it) is used as it is; host
    values go up through page-locked memory; the kernels clamp them to [0, F].

    ``rate``: a float, or a host sequence of B floats, each in [1 / 8, 8].  ``symbol_rates`` float32 [B, T_in] on the device gives
    every SYMBOL a rate instead: frame f of entry b takes ``symbol_rates[b, path[b, f]]`` clamped to [min_rate, max_rate]
    (+-inf, 0 and negative values clamp; a NaN, and a frame whose path value lies outside the entry's ``input_lengths``, is at rate
    1).  It needs ``path`` int32 [B, >= F] (``alignment_report``'s) and ``rate`` = 1 - fold a global factor into the table.  With
    ``path`` the result also carries every symbol's first and last frame; ``n_symbols`` (T_in) is needed where neither a table nor
    host ``input_lengths`` tells it.

    ``cap``: the frames of the result.  Default: the exact longest warped entry where rates and lengths are host values; the
    longest there could be - ``warped_length(F, rate)``, or ``warped_length(F, min_rate)`` for a table - otherwise.  A shorter cap
    cuts the entries to it.

    Returns WarpedMel(mel, lengths, cum, first_last, host_lengths):
      mel           [B, C, cap] of mel's dtype, dense: entry b's warped frames, +0 behind lengths[b]
      lengths       int32 [B] on the device: the warped frames F'
      cum           int64 [B, F + 1] on the device: the cumulative map c, source frame f covers [c[f], c[f+1]) / 2^20 output frames
      first_last    int32 [B, T_in, 2] on the device, or None without ``path``: a symbol's first and last frame, (-1, -1) for none
      host_lengths  int64 [B] on the host where rates and lengths were host values - ``warped_length`` of each, no read-back -
                    else None: what ``WaveGlow.infer_batch`` takes

    At rate 1 the result is the input bit for bit.  An output frame is the linear interpolation of the two source frames whose
    centres it lies between (np.interp at the frame centres of the cumulative map, ends clamped), formed in double and rounded once;
    an entry's bits are the same alone and at any place in a batch.  Two launches (the map, the gather) and a memset where there is a
    path, on the caller's current stream; nothing is read back and no arithmetic runs on the values outside the kernels."""
    who = "warp_mel"
    T2SError = _lib.T2SError
    if not (torch.is_tensor(mel) and mel.is_cuda):
        raise T2SError("%s: expected a mel in HBM (cuda); there is no CPU path" % who)
    if mel.dim() != 3 or mel.numel() == 0:
        raise T2SError("%s: mel must be [B, C, F] and hold values, got %s" % (who, tuple(mel.shape)))
    x = mel.detach()
    if x.dtype not in _KINDS:
        raise T2SError("%s: expected float32 or float16, got %s (there is no silent cast)" % (who, x.dtype))
    B, C, F = x.shape
    if B > 65535 or F > 2 ** 30:
        raise T2SError("%s: %d entries of %d frames, the most is 65535 of 2^30" % (who, B, F))
    dev = x.device
    lo, hi = _clamp_rates(min_rate, max_rate, who)
    stretches = _stretches(rate, B, who)
    if symbol_rates is not None and any(s != Q for s in stretches):
        raise ValueError("%s: with symbol_rates, rate must be 1 (fold a global factor into the table)" % who)
    path, ld_path, rates, ld_rates, in_len, T_in = _path_args(path, symbol_rates, input_lengths, n_symbols, B, F, dev, who)
    lens_d, lens_h = _lengths(lengths, B, F, dev, who, "lengths")
    exact = lens_h is not None and rates is None
    if cap is None:
        if exact:
            cap = max(1, max(_warped(int(n), s) for n, s in zip(lens_h.tolist(), stretches)))
        else:
            cap = max(_warped(F, s) for s in stretches) if rates is None else _warped(F, stretch_q(lo))
    else:
        try:
            cap = None if isinstance(cap, bool) else operator.index(cap)
        except TypeError:
            cap = None
        if cap is None or cap < 1:
            raise ValueError("%s: cap must be an integer >= 1" % who)
    if cap > 2 ** 31 - 1:
        raise T2SError("%s: %d output frames, the most is 2^31 - 1" % (who, cap))
    ld_row = x.stride(1) if C > 1 else F
    ld_entry = x.stride(0) if B > 1 else C * ld_row
    if x.stride(2) != 1 or ld_row < F or ld_entry < C * ld_row:
        x = x.contiguous()
        ld_row, ld_entry = F, C * F
    cum, out_len, fl = _map(dev, B, F, lens_d, stretches, cap, path, ld_path, rates, ld_rates, in_len, T_in, lo, hi)
    p = _lib.ptr
    with torch.cuda.device(dev):
        out = torch.empty(B, C, cap, dtype=x.dtype, device=dev)
        _lib.call("t2s_warp_gather", p(x), _KINDS[x.dtype], B, C, F, ld_row, ld_entry, p(lens_d), p(cum), p(out_len), p(out), cap,
                  _lib.current_stream())
    host = torch.tensor([_warped(int(n), s, cap) for n, s in zip(lens_h.tolist(), stretches)], dtype=torch.int64) if exact else None
    return WarpedMel(out, out_len, cum, fl, host)


def symbol_spans(warped_or_cum, path, input_lengths, lengths, hop, *, trim_bounds=None, offsets=None, ratio=(1, 1), total=None,
                 n_symbols=None):
    """[start, end) of every symbol in samples, read from a warp's cumulative map on the device.

    ``warped_or_cum``: a ``WarpedMel`` (its ``first_last`` is used where it has one), or the map itself, int64 [B, F + 1].
    ``path`` int32 [B, >= F] (``alignment_report``'s; not needed where a WarpedMel carries first_last), ``input_lengths`` and
    ``lengths`` [B] the symbols and the SOURCE frames of every entry (host or device; None: all), ``hop`` the vocoder's samples per
    frame.  Symbol k of entry b spans the output frames c[first] .. c[last + 1] of its first and last source frame; in samples
    u = (c hop) >> 20, so with a monotone path neighbouring spans abut exactly.  Then, each where given and in this order:

      trim_bounds  (start, end), int64 [B] each on the device - ``Trimmer.bounds_batch``'s: u = clamp(u - start, 0, end - start)
      offsets      int64 [B] on the device (or host integers): u += offsets[b], e.g. ``join_batches``' offsets by row
      ratio, total (up, down) of a ``Resampler`` and the utterance's length (an int, or a one-element device tensor such as the
                   ``length`` that ``resample_batch`` returns): u = min(u up // down, total)

    Returns int64 [B, T_in, 2] on the device, (-1, -1) for a symbol no frame attends to, for one at or behind the entry's
    input length and for every symbol of an entry without frames.  One launch (two and a memset where first / last have to be found
    first) on the caller's current stream; nothing is read back."""
    who = "symbol_spans"
    from .audio import _to_device
    T2SError = _lib.T2SError
    fl = None
    if isinstance(warped_or_cum, WarpedMel):
        cum, fl = warped_or_cum.cum, warped_or_cum.first_last
    else:
        cum = warped_or_cum
    if not (torch.is_tensor(cum) and cum.is_cuda and cum.dtype == torch.int64 and cum.dim() == 2 and cum.size(1) >= 2):
        raise T2SError("%s: expected a WarpedMel or its cumulative map, int64 [B, F + 1] in HBM" % who)
    cum = cum.detach().contiguous()
    B, F = cum.size(0), cum.size(1) - 1
    dev = cum.device
    try:
        hop, up, down = (0 if isinstance(v, bool) else operator.index(v) for v in (hop,) + tuple(ratio))
    except (TypeError, ValueError):
        hop = up = down = 0
    if not (1 <= hop <= Q and 1 <= up <= Q and 1 <= down <= Q) or F * hop > 2 ** 39:
        raise ValueError("%s: hop and ratio = (up, down) must be integers in [1, 2^20], F hop at most 2^39" % who)
    lens_d, _ = _lengths(lengths, B, F, dev, who, "lengths")
    if fl is None:
        if path is None:
            raise T2SError("%s: needs path (alignment_report's), or a WarpedMel made with one" % who)
        path, ld_path, _, _, in_len, T_in = _path_args(path, None, input_lengths, n_symbols, B, F, dev, who)
        _, _, fl = _map(dev, B, F, lens_d, [Q] * B, 1, path, ld_path, None, 0, in_len, T_in, want_cum=False)
    else:
        T_in = fl.size(1)
        in_len, _ = _lengths(input_lengths, B, T_in, dev, who, "input_lengths")

    def per_entry(t, what):
        if not torch.is_tensor(t):
            t = _to_device(torch.as_tensor(t, dtype=torch.int64), dev)
        if not (t.is_cuda and t.device == dev and t.dim() == 1 and t.numel() == B and t.dtype in (torch.int32, torch.int64)):
            raise T2SError("%s: %s must be %d integers on %s" % (who, what, B, dev))
        return t.detach().to(torch.int64).contiguous()
    t0 = t1 = off = total_d = None
    if trim_bounds is not None:
        t0, t1 = (per_entry(t, "trim_bounds") for t in trim_bounds)
    if offsets is not None:
        off = per_entry(offsets, "offsets")
    if torch.is_tensor(total):
        if not (total.is_cuda and total.device == dev and total.numel() == 1 and total.dtype in (torch.int32, torch.int64)):
            raise T2SError("%s: total must be an integer or a one-element integer tensor on %s" % (who, dev))
        total_d, total = total.detach().reshape(1).to(torch.int64), 0
    elif total is None:
        total = NO_TOTAL
    else:
        total = operator.index(total)
        if total < 0:
            raise ValueError("%s: total must not be negative" % who)
    p = _lib.ptr
    with torch.cuda.device(dev):
        spans = torch.empty(B, T_in, 2, dtype=torch.int64, device=dev)
        _lib.call("t2s_warp_spans", p(cum), p(fl), B, F, T_in, p(in_len), p(lens_d), hop, p(t0), p(t1), p(off), up, down, total,
                  p(total_d), p(spans), _lib.current_stream())
    return spans


class WarpStream:
    """``warp_mel`` at one rate for all entries, pushed piece by piece while the mel is still decoded (csrc/warp.hip).

    ``n_mel`` channels, ``capacity`` source frames at most (the decoder's max_decoder_steps), ``dtype`` float32 or float16,
    ``rate`` in [1 / 8, 8].  ``push(mel_piece [B, n_mel, n], last, rate=None)`` returns the warped frames that became settled -
    [B, n_mel, n'], possibly empty - and on the push flagged ``last`` everything up to ``warped_length``; the concatenation of the
    pieces is ``warp_mel(whole, None, rate).mel`` bit for bit, and the input itself at rate 1.  ``rate=`` applies to the frames of
    this push and of later ones, so the rate can change while the stream runs: the pieces are then ``warp_mel(whole, path=piece
    index of every frame, symbol_rates=the rates)``.  The host mirrors the cumulative map in exact integers from the stretches it
    passed, so it knows ``settled_length`` - and with it every shape - without a read-back: a push is two launches on the caller's
    current stream and no wait.

    Attributes: ``frames_in``, ``frames_out``; ``cum`` int64 [B, capacity + 1] on the device, valid up to column ``frames_in``;
    ``first_last`` int32 [B, n_symbols, 2] where a ``path`` was given (int32 [B, >= capacity] on the device, e.g. an
    ``AlignmentStream``'s, which must hold a frame's symbol before the frame is pushed here): ``symbol_spans`` reads both, with
    lengths = ``frames_in``.  The source mel known so far is kept in HBM (``streaming._MelBuffer``, as ``stream_windows`` keeps it)."""

    def __init__(self, n_mel, capacity, dtype, device, rate=1.0, *, B=1, path=None, n_symbols=None, input_lengths=None):
        from .streaming import _MelBuffer
        who = "WarpStream"
        T2SError = _lib.T2SError
        try:
            n_mel, capacity, B = (None if isinstance(v, bool) else operator.index(v) for v in (n_mel, capacity, B))
        except TypeError:
            n_mel = None
        if n_mel is None or n_mel < 1 or capacity < 1 or capacity > 2 ** 30 or not 1 <= B <= 65535:
            raise ValueError("%s: n_mel, capacity and B must be integers >= 1, capacity at most 2^30 and B at most 65535" % who)
        if dtype not in _KINDS:
            raise T2SError("%s: expected float32 or float16, got %s (there is no silent cast)" % (who, dtype))
        dev = torch.device(device)
        if dev.type != "cuda":
            raise T2SError("%s: the stream lives in HBM (cuda); there is no CPU path" % who)
        self.n_mel, self.capacity, self.dtype, self.device, self.B = n_mel, capacity, dtype, dev, B
        self.rate = rate
        self._path, self._ld_path, self._in_len, self.n_symbols = None, 0, None, 0
        self.first_last = None
        if path is not None:
            self._path, self._ld_path, _, _, self._in_len, self.n_symbols = _path_args(path, None, input_lengths, n_symbols, B, capacity,
                                                                                      dev, who)
            if self._path.data_ptr() != path.data_ptr():
                raise T2SError("%s: path must be dense along the frames (it is read again at every push)" % who)
        with torch.cuda.device(dev):
            self.cum = torch.empty(B, capacity + 1, dtype=torch.int64, device=dev)
            if path is not None:
                self.first_last = torch.empty(B, self.n_symbols, 2, dtype=torch.int32, device=dev)
        self._mel = _MelBuffer()
        self._c = [0, 0]                # c[n - 1], c[n] of the map, mirrored on the host
        self.frames_in = self.frames_out = 0
        self.ended = False
        self._order = _lib.StreamOrder()

    @property
    def rate(self):
        return self._rate

    @rate.setter
    def rate(self, value):
        self._stretch = stretch_q(value)
        self._rate = float(value)

    def push(self, mel_piece, last, rate=None):
        who = "WarpStream.push"
        T2SError = _lib.T2SError
        if self.ended:
            raise T2SError("%s: a piece arrived behind the one flagged last" % who)
        if rate is not None:
            self.rate = rate
        if not (torch.is_tensor(mel_piece) and mel_piece.is_cuda and mel_piece.device == self.device):
            raise T2SError("%s: expected a mel piece on %s" % (who, self.device))
        x = mel_piece.detach()
        if x.dim() != 3 or x.size(0) != self.B or x.size(1) != self.n_mel or x.dtype != self.dtype:
            raise T2SError("%s: a mel piece must be [%d, %d, n] %s, got %s %s" % (who, self.B, self.n_mel, self.dtype, tuple(x.shape), x.dtype))
        n0 = self.frames_in
        n = n0 + x.size(2)
        if n > self.capacity:
            raise T2SError("%s: %d frames, the stream was made for %d" % (who, n, self.capacity))
        cur = self._order.enter(self.device)
        if self._order.switched:
            _lib.record_stream((self.cum, self.first_last, self._mel.buf), cur)
        p, st, s = _lib.ptr, _lib.current_stream(), self._stretch
        with torch.cuda.device(self.device):
            if n > n0:
                self._mel.append(x)
                _lib.call("t2s_warp_window_map", self.B, self.capacity, n0, n, s, None, p(self._path), self._ld_path, p(self._in_len),
                          self.n_symbols, p(self.cum), p(self.first_last), st)
                self._c = [self._c[1] + (n - n0 - 1) * s, self._c[1] + (n - n0) * s]
            self.frames_in = n
            j0 = self.frames_out
            j1 = max(j0, settled_length(self._c[0], self._c[1], final=bool(last)))
            out = torch.empty(self.B, self.n_mel, j1 - j0, dtype=self.dtype, device=self.device)
            if j1 > j0:
                buf = self._mel.buf
                _lib.call("t2s_warp_window_gather", p(buf), _KINDS[self.dtype], self.B, self.n_mel, self.capacity, n, buf.stride(1),
                          buf.stride(0), p(self.cum), j0, j1, p(out), st)
        self.frames_out = j1
        self.ended = bool(last)
        return out
