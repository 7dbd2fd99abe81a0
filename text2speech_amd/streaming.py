"""Streaming synthesis: vocode windows of a mel while the rest of it is still decoded.

WaveGlow's inverse flow has a finite reach, and every keyed noise value is a function of (seed, channel, column) alone
(sampling.py), so a window of an utterance's frames, vocoded alone with enough frames on either side - the halo - and the draws of
its own columns, gives the audio the whole call gives for those frames.  ``vocoder_halo`` is that reach in frames, ``plan_windows``
the schedule (pure host arithmetic), ``WaveGlow.infer_window`` / ``infer_stream`` the vocoder side, ``Tacotron.inference_stream`` the
decoder side and ``synthesize_stream`` the two chained on one stream."""
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


def synthesize_stream(tacotron, waveglow, ids, speaker_id=None, seed=None, sigma=0.666, denoiser=None, strength=0.1, first_frames=32,
                      window_frames=128, halo=None, pcm16=False, delivery=None):
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
    for bit.  A push that gives nothing yields nothing.  Not together with ``pcm16`` (the stream has its own encoding); the
    speaking rate, timestamps and the alignment check are not part of a stream."""
    if tacotron.training or waveglow.training:
        raise _lib.T2SError("synthesize_stream runs in eval mode only (call .eval() on both models)")
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
    return _synthesize(mels, waveglow, seed, sigma, denoiser, strength, first_frames, window_frames, halo, margin, stride, pcm16,
                       delivery)


def _synthesize(mels, waveglow, seed, sigma, denoiser, strength, first_frames, window_frames, halo, margin, stride, pcm16,
                delivery=None):
    from . import audio as A
    pieces = ((p[1], p[4]) for p in mels)
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
