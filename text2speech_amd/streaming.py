"""Streaming synthesis: vocode windows of a mel while the rest of it is still decoded.

WaveGlow's inverse flow has a finite reach, and every keyed noise value is a function of (seed, channel, column) alone
(sampling.py), so a window of an utterance's frames, vocoded alone with enough frames on either side - the halo - and the draws of
its own columns, gives the audio the whole call gives for those frames.  ``vocoder_halo`` is that reach in frames, ``plan_windows``
the schedule (pure host arithmetic), ``WaveGlow.infer_window`` / ``infer_stream`` the vocoder side, ``Tacotron.inference_stream`` the
decoder side and ``synthesize_stream`` the two chained on one stream.  ``StreamControl`` is what its ``control=`` takes: the speaking
rate (``rate.WarpStream``), symbol timestamps and the alignment watchdog (``alignment.AlignmentStream``) inside the stream."""
import torch

from . import _lib

UPSAMPLE_KERNEL, UPSAMPLE_STRIDE = 1024, 256        # glow.WaveGlow's ConvTranspose1d, fixed there as in the reference


def vocoder_halo(waveglow_or_cfg):
    """(left, right): the frames in front of and behind a window that decide its audio.  Each WN sees +-(2^n_layers - 1)
    (kernel_size - 1) / 2 columns and the flows are chained, so n_flows times that many columns, at stride / n_group columns per
    frame:  right = ceil(n_flows reach / (stride / n_group));  the transposed convolution of the upsampler additionally reaches
    ceil((kernel - stride) / stride) frames back:  left = right + that.  (99, 96) at the defaults.  Takes a WaveGlow or the dict
    it is built from; raises T2SError where stride % n_group != 0 (a frame is then no whole number of columns)."""
    if isinstance(waveglow_or_cfg, dict):
        cfg = waveglow_or_cfg
        n_flows, G = int(cfg["n_flows"]), int(cfg["n_group"])
        nl, ks = int(cfg["WN_config"]["n_layers"]), int(cfg["WN_config"]["kernel_size"])
        kernel, stride = UPSAMPLE_KERNEL, UPSAMPLE_STRIDE
    else:
        m = waveglow_or_cfg
        n_flows, G = int(m.n_flows), int(m.n_group)
        nl, ks = int(m.WN[0].n_layers), int(m.WN[0].kernel_size)
        kernel, stride = int(m.upsample.kernel_size[0]), int(m.upsample.stride[0])
    if stride % G:
        raise _lib.T2SError("streaming needs the upsampler's stride (%d) to be a multiple of n_group (%d)" % (stride, G))
    reach = (2 ** nl - 1) * (ks - 1) // 2
    cols = stride // G
    right = -(-n_flows * reach // cols)
    left = right + -(-max(0, kernel - stride) // stride)
    return left, right


def plan_windows(first_frames, window_frames, halo, n_known, end=False, start=0):
    """The next window of a stream, or None where it cannot be issued yet (or nothing is left).  ``n_known`` frames 0 .. n_known - 1
    are decoded, ``end``: n_known is the utterance's length; ``start``: the first frame no window has delivered yet (the f1 of the
    window before, 0 at first).  Returns (f0, f1, lo, hi): the window delivers frames [f0, f1) and is computed on [lo, hi).

    Frames are delivered in order, each by exactly one window: [0, first_frames), then runs of window_frames, the last one cut at
    the end.  A window is issued only once hi <= n_known, or the end is known.  The computed regions have at most three lengths:
      the first window     [0, first_frames + right), cut at the end where that is known;
      a regular window     W = left + window_frames + right frames, [f0 - left, f1 + right) - or [0, W) while f0 < left: such a
                           window waits until W frames are decoded (more context than it needs) and keeps the one length;
      once the end is known  hi = min(F, max(f1 + right, W)) and lo = max(0, hi - W): min(W, F) frames, whatever is left.
    A longer region than the halo asks for never changes the result: the halo is the reach, and what lies beyond it has no
    influence."""
    left, right = int(halo[0]), int(halo[1])
    first_frames, window_frames, n_known, start = int(first_frames), int(window_frames), int(n_known), int(start)
    if first_frames < 1 or window_frames < 1 or left < 0 or right < 0 or start < 0 or n_known < 0:
        raise ValueError("plan_windows: first_frames and window_frames must be >= 1, the halo, start and n_known >= 0")
    if end and start >= n_known:
        return None
    if start == 0:
        f1 = first_frames
        hi = f1 + right
        if end:
            f1, hi = min(f1, n_known), min(hi, n_known)
        elif hi > n_known:
            return None
        return 0, f1, 0, hi
    W = left + window_frames + right
    f1 = start + window_frames
    hi = max(f1 + right, W)
    if end:
        f1, hi = min(f1, n_known), min(hi, n_known)
    elif hi > n_known:
        return None
    return start, f1, max(0, hi - W), hi


class _MelBuffer:
    """The frames of an utterance known so far, [B, n_mel, capacity] on the device, grown by doubling."""

    def __init__(self):
        self.buf = None
        self.n = 0

    def append(self, piece):
        n = piece.size(2)
        if self.buf is None:
            cap = max(256, 2 * n)
            self.buf = torch.empty(piece.size(0), piece.size(1), cap, dtype=piece.dtype, device=piece.device)
        elif self.n + n > self.buf.size(2):
            grown = torch.empty(self.buf.size(0), self.buf.size(1), max(2 * self.buf.size(2), self.n + n), dtype=self.buf.dtype,
                                device=self.buf.device)
            grown[:, :, :self.n] = self.buf[:, :, :self.n]
            self.buf = grown
        self.buf[:, :, self.n:self.n + n] = piece
        self.n += n

    def known(self):
        return self.buf[:, :, :self.n]


def _check_stream_args(waveglow, seed, first_frames, window_frames, halo, who):
    if seed is None:
        raise _lib.T2SError("%s: a seed is required - a window's draws are keyed by (seed, channel, column)" % who)
    exact = vocoder_halo(waveglow)
    if halo is None:
        halo = exact
    halo = (int(halo[0]), int(halo[1]))
    if halo[0] < 0 or halo[1] < 0:
        raise ValueError("%s: halo must be (left, right) >= 0, got %r" % (who, halo))
    if int(first_frames) < 1 or int(window_frames) < 1:
        raise ValueError("%s: first_frames and window_frames must be >= 1" % who)
    return halo


def stream_windows(waveglow, pieces, sigma, seed, first_frames, window_frames, halo, margin=0, who="infer_stream", flag_last=False):
    """The generator behind ``WaveGlow.infer_stream``: over (mel piece [B, n_mel, n], last) it yields (audio [B, stride (g1 - g0)],
    f0, f1, g0, g1) per window, where the window delivers frames [f0, f1) and the audio covers [g0, g1) = [f0 - margin, f1 + margin)
    clipped to the utterance (margin > 0: synthesize_stream's denoiser wants its STFT's reach around every inner edge).  With
    ``flag_last`` a sixth value says whether the window is the utterance's last.  The workspaces of the windows' shapes live in a
    dict of this generator, at most three (``_Engine.workspace``)."""
    left, right = halo
    plan_halo = (left + margin, right + margin)
    mel = _MelBuffer()
    ws = {}
    start = 0
    ended = False
    for piece, last in pieces:
        if ended:
            raise _lib.T2SError("%s: a piece arrived behind the one flagged last" % who)
        if piece.dim() != 3:
            raise _lib.T2SError("%s: a mel piece must be [B, n_mel, n], got %s" % (who, tuple(piece.shape)))
        if piece.size(2):
            mel.append(piece)
        ended = bool(last)
        if mel.n == 0:
            continue
        while True:
            win = plan_windows(first_frames, window_frames, plan_halo, mel.n, ended, start)
            if win is None:
                break
            f0, f1, lo, hi = win
            g0, g1 = max(0, f0 - margin), (min(mel.n, f1 + margin) if ended else f1 + margin)
            audio = waveglow.infer_window(mel.known(), g0, g1, sigma=sigma, seed=seed, final=ended, halo=halo, _region=(lo, hi),
                                          _ws=ws)
            start = f1
            yield (audio, f0, f1, g0, g1, ended and f1 >= mel.n) if flag_last else (audio, f0, f1, g0, g1)
    if not ended:
        raise _lib.T2SError("%s: the pieces ended without one flagged last" % who)


class StreamControl:
    """What ``synthesize_stream(control=)`` takes - one per utterance, or a callable without arguments that makes one - and the side
    channel the caller reads between pieces and afterwards; the stream keeps yielding bare audio tensors.

      speed       None, or a rate in [1 / 8, 8]: every mel_post piece goes through a ``rate.WarpStream`` between the two models, and
                  the audio is ``infer(warp_mel(mel_post, speed).mel)``'s.  ``ctl.speed = x`` between pieces takes effect from the
                  next mel piece on (a stream that began with ``speed=None`` and without timestamps has no warp to change)
      check       None, or an ``alignment.AlignmentCheck``: every alignment piece goes through an ``alignment.AlignmentStream``,
                  whose live flags - SKIP, BACK, STALL, NONFINITE - are copied to page-locked memory behind every piece.  The
                  flags of piece k are read before anything of piece k + 1 is issued; the decoder's stop poll in between has
                  already waited for that stream, so the read adds no wait
      on_fail     "stop": on non-zero flags piece k + 1 is discarded, the decoder is closed and the utterance ends at the last
                  frame whose mel_post had been yielded through piece k - the vocoder's last windows and the delivery are flushed
                  as at an utterance's end, and ``aborted`` is True.  "flag": the flags are only recorded
      timestamps  True: the warp's cumulative map and every symbol's first and last frame are kept on the device, and ``spans()``
                  reads them

    Readable at any time: ``frames_in`` / ``frames_out`` (mel_post frames taken and frames handed to the vocoder), ``flags`` (host
    int, the latest read), ``aborted``, ``path`` (int32 [1, frames] on the device), ``report()`` (an ``AlignmentReport`` of the
    prefix, on the device) and ``spans(ratio, total)``."""

    def __init__(self, speed=None, check=None, on_fail="stop", timestamps=False):
        from .alignment import AlignmentCheck
        if check is not None and not isinstance(check, AlignmentCheck):
            raise _lib.T2SError("StreamControl: check must be an alignment.AlignmentCheck or None, got a %s" % type(check).__name__)
        if on_fail not in ("stop", "flag"):
            raise ValueError("StreamControl: on_fail must be \"stop\" or \"flag\", got %r" % (on_fail,))
        if not isinstance(timestamps, bool):
            raise ValueError("StreamControl: timestamps must be True or False, got %r" % (timestamps,))
        self.check, self.on_fail, self.timestamps = check, on_fail, timestamps
        self._speed = None
        self._align = self._warp = None
        self._began = False
        self.speed = speed
        self.frames_in = self.frames_out = 0
        self.flags = 0
        self.aborted = False

    @property
    def speed(self):
        return self._speed

    @speed.setter
    def speed(self, value):
        from .rate import stretch_q
        if value is None:
            if self._began and self._warp is not None:
                raise ValueError("StreamControl: the stream warps already; speed=None cannot be set while it runs (1.0 is the identity)")
        else:
            stretch_q(value)                # (raises ValueError on anything but a rate in [1 / 8, 8])
            if self._began and self._speed is None and not self.timestamps:
                raise _lib.T2SError("StreamControl: the stream began with speed=None and has no warp to change; begin it with speed=1.0")
            value = float(value)
        self._speed = value

    def _begin(self, capacity, stride):
        if self._began:
            raise _lib.T2SError("synthesize_stream: a StreamControl serves one utterance (pass a callable that makes one per call)")
        self._began = True
        self._capacity, self._stride = int(capacity), int(stride)

    def _feed(self, piece):
        """one decoder piece -> the mel piece the vocoder takes"""
        from .alignment import AlignmentCheck, AlignmentStream
        from .rate import WarpStream
        _, mel, _, align, last = piece
        dev = mel.device
        if self._align is None and (self.check is not None or self.timestamps):
            off = AlignmentCheck(-1, -1, -1, -1, 0.0, 0)           # timestamps alone: the path is wanted, no bit is
            self._align = AlignmentStream(self.check if self.check is not None else off, align.size(2), self._capacity, dev)
        if self._align is not None:
            self._align.push(align, last)
        if self._warp is None and (self._speed is not None or self.timestamps):
            path = self._align.path if self.timestamps else None
            self._warp = WarpStream(mel.size(1), self._capacity, mel.dtype, dev, 1.0 if self._speed is None else self._speed,
                                    path=path, n_symbols=align.size(2) if self.timestamps else None)
        self._empty = mel[:, :, :0]
        out = mel if self._warp is None else self._warp.push(mel, last, rate=self._speed)
        self.frames_in += mel.size(2)
        self.frames_out += out.size(2)
        return out

    def _read_flags(self):
        """the flags of the latest alignment piece, from page-locked memory -> whether the stream has to stop"""
        if self._align is None or self.check is None or not self._align.pushes:
            return False
        self.flags = int(self._align.wait()[0][0])
        self.aborted = bool(self.flags) and self.on_fail == "stop" and not self._align.ended
        return self.aborted

    def _flush(self):
        """the utterance ends here: what the warp still holds back"""
        if self._warp is None:
            return self._empty
        out = self._warp.push(self._empty, True)
        self.frames_out += out.size(2)
        return out

    @property
    def path(self):
        if self._align is None:
            raise _lib.T2SError("StreamControl.path: needs check= or timestamps=True, and a first piece")
        return self._align.path[:, :self._align.frames]

    def report(self):
        if self._align is None:
            raise _lib.T2SError("StreamControl.report: needs check= or timestamps=True, and a first piece")
        return self._align.report()

    def spans(self, ratio=(1, 1), total=None):
        """int64 [1, T_in, 2] on the device: every symbol's [start, end) so far, in samples of the audio the stream delivers -
        ``rate.symbol_spans`` over the stream's own map with hop = the vocoder's stride, ``ratio`` = (up, down) of the delivery's
        resampler and ``total`` its length where known.  A symbol no frame has attended to yet is (-1, -1)."""
        from .rate import WarpedMel, symbol_spans
        if not self.timestamps:
            raise _lib.T2SError("StreamControl.spans: the control was made with timestamps=False")
        if self._warp is None:
            raise _lib.T2SError("StreamControl.spans: no piece has been decoded yet")
        w = self._warp
        return symbol_spans(WarpedMel(None, None, w.cum, w.first_last, None), None, None, [w.frames_in], self._stride, ratio=ratio,
                            total=total)


def _control_pieces(mels, ctl):
    """inference_stream's pieces through a StreamControl -> (mel piece, last) for stream_windows"""
    for piece in mels:
        if ctl._read_flags():               # piece k's flags, before anything of piece k + 1 is issued: k + 1 is discarded
            mels.close()
            yield ctl._flush(), True
            return
        yield ctl._feed(piece), piece[4]
    ctl._read_flags()


def synthesize_stream(tacotron, waveglow, ids, speaker_id=None, seed=None, sigma=0.666, denoiser=None, strength=0.1, first_frames=32,
                      window_frames=128, halo=None, pcm16=False, delivery=None, control=None):
    """Text to audio pieces: ``tacotron.inference_stream`` feeding ``waveglow.infer_stream`` on one stream.  A generator of audio
    pieces [1, n] (float32, or int16 with ``pcm16``) whose concatenation is the utterance; the first one exists once
    first_frames + halo frames are decoded, not after the last frame.  ``seed`` (required) keys both the prenet masks and the
    vocoder's noise, as ``inference(seed=)`` and ``infer(seed=)`` take it.  The next decode chunk is enqueued before a vocoder
    window (inference_stream's order) and its stop step polled behind it, so the device does not idle through the poll.

    Without ``denoiser`` the audio is ``infer_stream`` fed the streamed mel_post, bit for bit.  With one, each vocoder window is
    widened by the STFT's reach, ceil(filter_length / stride) = 4 frames per inner edge; ``denoiser.forward(., strength)`` runs on
    the widened window and the centre is kept, so every kept sample sees the samples the whole-utterance call shows it, and the
    utterance's own ends keep their reflect padding.  B = 1, eval mode; ``halo`` as ``infer_window`` takes it.  Arguments are
    checked here, before the first piece is asked for.

    ``delivery``: an ``audio.DeliveryStream`` (one per utterance), or a callable without arguments that makes one.  Every piece -
    denoised where there is a denoiser - is pushed through it, the last one flagged, and what comes out is yielded: resampled,
    limited and encoded audio whose concatenation is the whole-utterance chain applied to the plain stream's concatenation, bit
    for bit.  A push that gives nothing yields nothing.  Not together with ``pcm16`` (the stream has its own encoding).

    ``control``: a ``StreamControl`` (one per utterance), or a callable without arguments that makes one: the speaking rate, symbol
    timestamps and the alignment watchdog inside the stream.  The chain is then inference_stream -> ``WarpStream.push`` of every
    mel_post piece -> the vocoder's windows -> denoiser -> delivery, with every alignment piece pushed into an ``AlignmentStream``;
    the control object is the side channel, the stream keeps yielding bare audio.  With ``control=None`` the call issues the
    launches it issued before.  Not part of a stream: per-symbol rate tables (their settled count is data on the device), a
    reaction inside the piece that failed (a host wait per chunk), decoding a failed stream again, B > 1, trimming."""
    if tacotron.training or waveglow.training:
        raise _lib.T2SError("synthesize_stream runs in eval mode only (call .eval() on both models)")
    if control is not None and not isinstance(control, StreamControl):
        if not callable(control):
            raise _lib.T2SError("synthesize_stream: control must be a streaming.StreamControl or a callable that makes one, got a %s"
                                % type(control).__name__)
        control = control()
        if not isinstance(control, StreamControl):
            raise _lib.T2SError("synthesize_stream: control() returned a %s, not a streaming.StreamControl" % type(control).__name__)
    if delivery is not None:
        if pcm16:
            raise _lib.T2SError("synthesize_stream: delivery= and pcm16=True exclude each other (ask the DeliveryStream for \"pcm16\")")
        from .audio import DeliveryStream
        if not isinstance(delivery, DeliveryStream):
            if not callable(delivery):
                raise _lib.T2SError("synthesize_stream: delivery must be an audio.DeliveryStream or a callable that makes one, got a %s"
                                    % type(delivery).__name__)
            delivery = delivery()
            if not isinstance(delivery, DeliveryStream):
                raise _lib.T2SError("synthesize_stream: delivery() returned a %s, not an audio.DeliveryStream" % type(delivery).__name__)
    halo = _check_stream_args(waveglow, seed, first_frames, window_frames, halo, "synthesize_stream")
    stride = int(waveglow.upsample.stride[0])
    margin = 0
    if denoiser is not None:
        if stride % denoiser.stft.hop_length:
            raise _lib.T2SError("synthesize_stream: the denoiser's hop (%d) must divide the vocoder's stride (%d)"
                                % (denoiser.stft.hop_length, stride))
        margin = -(-denoiser.stft.filter_length // stride)
    mels = tacotron.inference_stream(ids, speaker_id, seed=seed)
    if control is not None:
        control._begin(tacotron.decoder.max_decoder_steps, stride)
    return _synthesize(mels, waveglow, seed, sigma, denoiser, strength, first_frames, window_frames, halo, margin, stride, pcm16,
                       delivery, control)


def _synthesize(mels, waveglow, seed, sigma, denoiser, strength, first_frames, window_frames, halo, margin, stride, pcm16,
                delivery=None, control=None):
    from . import audio as A
    pieces = ((p[1], p[4]) for p in mels) if control is None else _control_pieces(mels, control)
    for audio, f0, f1, g0, g1, last in stream_windows(waveglow, pieces, sigma, seed, first_frames, window_frames, halo, margin,
                                                      "synthesize_stream", flag_last=True):
        if denoiser is not None:
            with torch.no_grad():
                audio = denoiser(audio, strength)[:, 0, stride * (f0 - g0):stride * (f1 - g0)]
        if delivery is None:
            yield A.to_pcm16(audio) if pcm16 else audio
            continue
        out = delivery.push(audio, last)
        if out.size(1):
            yield out
    if delivery is not None and control is not None and control.aborted and not delivery._ended:
        # (the watchdog cut the utterance at a frame the windows had already delivered: the delivery still ends as one ends)
        out = delivery.push(control._empty.new_empty(control._empty.size(0), 0, dtype=torch.float32), True)
        if out.size(1):
            yield out
