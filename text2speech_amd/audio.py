"""Audio front-end / back-end on the MI355X, behind the reference's own class surface:

  STFT(filter_length, hop_length, win_length, window)        utils/stft.py:36-134      .transform / .inverse / .forward
  TacotronSTFT(filter_length, hop_length, win_length, n_mel_channels, sampling_rate, mel_fmin, mel_fmax)
                                                             utils/layers.py:42-79     .mel_spectrogram
  Denoiser(waveglow, filter_length, n_overlap, win_length, mode)   waveglow/denoiser.py:7-40   .forward(audio, strength)
  dynamic_range_compression / _decompression                 utils/audio_processing.py:78-93

All arithmetic after construction runs in libt2s_hip.so (csrc/audio_ops.hip + the GEMV / f32 matrix-core GEMM of the
Tacotron path); there is no CPU or eager fallback - without the library every call raises.  The reference bounces the
waveform host -> GPU -> host inside STFT.transform (utils/stft.py:85-89); here input and output stay in HBM.
Padded batches of different lengths go through the *_batch methods (STFT.transform_batch / inverse_batch,
TacotronSTFT.mel_spectrogram_batch, Denoiser.denoise_batch) and to_pcm16: every entry gets what the plain method gives it alone, bit
for bit, and zeros behind its end.  from_pcm16 is to_pcm16's inverse; training batches from a pool of int16
clips are text2speech_amd/data.py.  Resampler converts the sample rate of a batch (forward / resample_batch) or, through
PcmPool.resample, of a pool: scipy.signal.resample_poly's polyphase filter with every sum in double precision (csrc/resample.hip).
Trimmer cuts leading and trailing silence (librosa.effects.trim's decision) and rescales to a peak, on a batch (forward /
trim_batch / bounds_batch) or, through PcmPool.rescale_trim, on a pool (csrc/trim.hip).  Loudness measures BS.1770 / EBU R128 gated
loudness and brings rows to a target level (measure_batch / normalize_batch; PcmPool.loudness / normalize_loudness for a pool;
csrc/loudness.hip).  Limiter is the chain's last stage, a true-peak meter and look-ahead limiter (true_peak_batch / limit_batch;
Loudness.normalize_limit_batch; PcmPool.true_peak / limit; csrc/limiter.hip).  DeliveryStream is that chain inside a stream: resample,
gain, limit and encode (float32, int16, G.711 through to_ulaw / to_alaw) piece by piece, the pieces' concatenation being the
whole-utterance chain's result bit for bit (csrc/delivery.hip; synthesize_stream(delivery=)).  join_batches / join_batch turn the padded
rows of such batches back into one utterance - pauses between them, ramps at the joints - with no length read back (csrc/join.hip;
text2speech_amd/longform.py is the chain around it).
Bases are built on the host at construction exactly as the reference builds them (numpy FFT of the identity, pinv, scipy
window); the mel filterbank restates librosa.filters.mel's defaults (Slaney scale, area normalisation) because librosa is
an unpinned dependency that this image does not have.
"""
import collections
import operator

import numpy as np
import torch
from scipy.signal import get_window

from . import _lib

__all__ = ["STFT", "TacotronSTFT", "Denoiser", "griffin_lim", "mel_filterbank", "dynamic_range_compression",
           "dynamic_range_decompression", "to_pcm16", "from_pcm16", "Resampler", "resample_filter", "Trimmer", "Loudness", "LoudnessReport",
           "loudness_coefficients", "Limiter", "LimiterReport", "limiter_window", "LIMIT_FLAG_LIMITED", "LIMIT_FLAG_NONFINITE",
           "LIMIT_MAX_LOOKAHEAD", "DeliveryStream", "DELIVERY_ENCODINGS", "to_ulaw", "to_alaw", "join_batches", "join_batch",
           "SosFilter", "FilterStream", "FilterReport", "sos_table", "sos_preemphasis", "sos_deemphasis", "sos_butter", "SOS_MAX_SECTIONS"]


def _ru(a, b):
    return -(-a // b) * b


def _need_cuda(t, what):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise RuntimeError("%s: expected a tensor in HBM (cuda); there is no CPU path" % what)


def _host_lengths(lengths, B, lo, hi, what, unit):
    """`lengths` (host or device tensor, or a sequence of integers) as a validated host int64 [B], every value in [lo, hi]: the
    checks of WaveGlow.infer_batch.  One read-back when they live on the device."""
    T2SError = _lib.T2SError
    try:
        lens = torch.as_tensor(lengths)
    except (TypeError, ValueError, RuntimeError) as e:
        raise T2SError("%s: lengths must be a tensor or a sequence of integers (%s)" % (what, e))
    if lens.is_floating_point() or lens.is_complex() or lens.dtype == torch.bool:
        raise T2SError("%s: lengths must be integers, got %s" % (what, lens.dtype))
    lens = lens.detach().to("cpu", torch.int64)
    if lens.dim() != 1 or lens.numel() != B:
        raise T2SError("%s: lengths has shape %s, the batch holds %d entries" % (what, tuple(lens.shape), B))
    if B == 0:
        raise T2SError("%s: an empty batch" % what)
    if int(lens.min()) < lo:
        b = int(lens.argmin())
        raise T2SError("%s: entry %d has %d %s, the minimum is %d (lengths %s)" % (what, b, int(lens[b]), unit, lo, lens.tolist()))
    if int(lens.max()) > hi:
        b = int(lens.argmax())
        raise T2SError("%s: entry %d has %d %s, the padded batch holds %d (lengths %s)" % (what, b, int(lens[b]), unit, hi,
                                                                                         lens.tolist()))
    return lens


def _to_device(host, dev):
    """A small host tensor -> the device through page-locked memory, without waiting for the copy (the caching host allocator keeps
    the staging block until the copy has run): what lets a batch be assembled with no synchronising call."""
    return host.pin_memory().to(dev, non_blocking=True)


def _both(lens, dev):
    """host int64 [B] -> (int32 on the device for the kernels, int32 on the host for the entry point's own reads)"""
    host = lens.to(torch.int32).contiguous()
    return _to_device(host, dev), host


def to_pcm16(audio, lengths=None):
    """Waveform in [-1, 1) -> int16 PCM on the device, the reference's `audio * 32768` then `astype('int16')` (truncation toward
    zero) - with saturation, which is a stated departure: numpy's cast of an out-of-range float is undefined, here +1.0 gives
    32767, anything beyond the range its nearest end, NaN 0.  `audio` [..., N] float32 or float16 in HBM; `lengths` (one per row,
    host or device or a sequence; None: every sample) zeroes the samples at and behind each row's end, which are not read.
    Returns an int16 tensor of audio's shape."""
    _need_cuda(audio, "to_pcm16")
    if audio.dim() == 0 or audio.numel() == 0:
        raise _lib.T2SError("to_pcm16: audio must hold samples, got shape %s" % (tuple(audio.shape),))
    x = audio.detach()
    if x.dtype not in (torch.float32, torch.float16):
        x = x.to(torch.float32)
    N = x.size(-1)
    rows = x.numel() // N
    if x.dim() == 2 and x.stride(1) == 1 and (rows == 1 or x.stride(0) >= N):
        ldx = x.stride(0) if rows > 1 else N                  # a view of wider rows goes in as it is
    else:
        x = x.contiguous()
        ldx = N
    lens_d = None
    if lengths is not None:
        lens_d, _ = _both(_host_lengths(lengths, rows, 0, N, "to_pcm16", "samples"), x.device)
    out = torch.empty(audio.shape, dtype=torch.int16, device=x.device)
    _lib.call("t2s_pcm16", _lib.ptr(x), int(x.dtype == torch.float16), rows, N, ldx, _lib.ptr(lens_d), _lib.ptr(out),
              _lib.current_stream())
    return out


def _pcm16_gather(pool, table, N, max_wav_value, out=None):
    """Rows of `N` float32 samples gathered from the flat int16 `pool` (in HBM) at `table` (host int64 [B, 2]: start, count), each
    divided by max_wav_value, zeros behind its count (t2s_pcm16_gather).  One small host-to-device copy, no read-back."""
    B = table.size(0)
    if out is None:
        out = torch.empty(B, N, dtype=torch.float32, device=pool.device)
    table_d = _to_device(table.contiguous(), pool.device)
    _lib.call("t2s_pcm16_gather", _lib.ptr(pool), pool.numel(), _lib.ptr(table_d), B, N, float(max_wav_value), _lib.ptr(out),
              out.stride(0) if B > 1 else N, _lib.current_stream())
    return out


def from_pcm16(pcm, lengths=None, max_wav_value=32768.0):
    """int16 PCM [..., N] in HBM -> float32 of the same shape, `pcm / max_wav_value`: to_pcm16's inverse (the round trip over all
    65536 codes is the identity; with max_wav_value = 32768 the division is exact).  `lengths` (one per row, as to_pcm16's) zeroes
    the samples at and behind each row's end."""
    _need_cuda(pcm, "from_pcm16")
    if pcm.dtype != torch.int16:
        raise _lib.T2SError("from_pcm16: expected int16 PCM, got %s (there is no silent cast)" % pcm.dtype)
    if pcm.dim() == 0 or pcm.numel() == 0:
        raise _lib.T2SError("from_pcm16: pcm must hold samples, got shape %s" % (tuple(pcm.shape),))
    if not (np.isfinite(max_wav_value) and max_wav_value > 0):
        raise _lib.T2SError("from_pcm16: max_wav_value must be finite and positive, got %r" % (max_wav_value,))
    x = pcm.detach().contiguous()
    N = x.size(-1)
    rows = x.numel() // N
    table = torch.empty(rows, 2, dtype=torch.int64)
    table[:, 0] = torch.arange(rows, dtype=torch.int64) * N
    table[:, 1] = N if lengths is None else _host_lengths(lengths, rows, 0, N, "from_pcm16", "samples")
    return _pcm16_gather(x.view(-1), table, N, max_wav_value).view(pcm.shape)


RESAMPLE_MAX_FACTOR = 512      # the library's limit on max(up, down) (include/t2s_hip.h)


def resample_filter(orig_rate, new_rate, half_width=10, beta=5.0):
    """(up, down, h) of scipy.signal.resample_poly(x, up, down) at its defaults (window=('kaiser', 5.0)): up / down is
    new_rate / orig_rate reduced, h float64 [2 half_width max(up, down) + 1] = up * firwin(n_taps, 1 / max(up, down), window).
    numpy only; the filter is scipy's, not librosa's kaiser_best or soxr."""
    if int(orig_rate) != orig_rate or int(new_rate) != new_rate or orig_rate < 1 or new_rate < 1 or half_width < 1:
        raise ValueError("resample_filter: rates and half_width must be positive integers, got %r, %r, %r"
                         % (orig_rate, new_rate, half_width))
    g = int(np.gcd(int(orig_rate), int(new_rate)))
    up, down = int(new_rate) // g, int(orig_rate) // g
    R = max(up, down)
    half = int(half_width) * R
    t = np.arange(-half, half + 1, dtype=np.float64) / R
    h = np.kaiser(2 * half + 1, beta) * (np.sinc(t) / R)
    return up, down, up * (h / h.sum())


class Resampler:
    """Sample-rate conversion orig_rate -> new_rate in HBM: scipy.signal.resample_poly(x, up, down) at its defaults (zero extension,
    Kaiser-windowed sinc of resample_filter) as one HIP kernel, every sum in double precision (csrc/resample.hip).  The filter lives
    in HBM from construction.  A reduced ratio with max(up, down) > 512 (e.g. 44100 -> 48000 is 160 / 147; 44100 -> 44101 is not
    supported) raises T2SError.  Equal rates give a copy without a launch of the filter."""

    def __init__(self, orig_rate, new_rate, half_width=10, beta=5.0, device="cuda"):
        self.orig_rate, self.new_rate = int(orig_rate), int(new_rate)
        self.up, self.down, h = resample_filter(orig_rate, new_rate, half_width, beta)
        if max(self.up, self.down) > RESAMPLE_MAX_FACTOR:
            raise _lib.T2SError("Resampler: %d -> %d Hz is the ratio %d / %d; max(up, down) may be at most %d"
                                % (orig_rate, new_rate, self.up, self.down, RESAMPLE_MAX_FACTOR))
        self.n_taps = h.size
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.T2SError("Resampler: the filter lives in HBM (cuda); there is no CPU path")
        self.h = torch.from_numpy(h).to(dev)

    def out_length(self, n):
        """samples that n input samples give: ceil(n up / down)"""
        return -(-int(n) * self.up // self.down)

    def _filter(self):
        return _lib.ptr(self.h), self.n_taps, self.up, self.down

    def _table(self, src, table, dst, max_out):
        """t2s_resample_table over `table` (host int64 [n, 4]: src_start, src_count, dst_start, dst_cap) from the flat device tensor
        `src` (int16 / f32 / f16) into the flat `dst` (int16 / f32), 65535 rows a launch."""
        kinds = {torch.int16: 0, torch.float32: 1, torch.float16: 2}
        table_d = _to_device(table.contiguous(), src.device)
        for r0 in range(0, table.size(0), 65535):
            rows = min(65535, table.size(0) - r0)
            _lib.call("t2s_resample_table", _lib.ptr(src), kinds[src.dtype], src.numel(), _lib.ptr(table_d[r0:]), rows,
                      *self._filter(), _lib.ptr(dst), kinds[dst.dtype], dst.numel(), int(max_out), None, _lib.current_stream())
        return dst

    def _rows(self, audio, what):
        """[N], [B, N] or [B, 1, N] f32 / f16 in HBM -> (rows [B, N] with unit stride inside a row, B, N, ldx)"""
        _need_cuda(audio, what)
        if audio.device != self.h.device:
            raise _lib.T2SError("%s: audio is on %s, the filter on %s" % (what, audio.device, self.h.device))
        if audio.dim() not in (1, 2, 3) or (audio.dim() == 3 and audio.size(1) != 1) or audio.numel() == 0:
            raise _lib.T2SError("%s: audio must be [N], [B, N] or [B, 1, N] and hold samples, got %s" % (what, tuple(audio.shape)))
        x = audio.detach()
        if x.dtype not in (torch.float32, torch.float16):
            raise _lib.T2SError("%s: expected float32 or float16, got %s (int16 pools go through PcmPool.resample)" % (what, x.dtype))
        N = x.size(-1)
        x = x.reshape(-1, N)
        B = x.size(0)
        if B > 65535:
            raise _lib.T2SError("%s: %d rows, the most is 65535" % (what, B))
        if x.stride(1) != 1 or (B > 1 and x.stride(0) < N):
            x = x.contiguous()
        return x, B, N, (x.stride(0) if B > 1 else N)

    def _batch(self, x, B, N, ldx, lens_d, want_lengths):
        n_out = self.out_length(N)
        out = torch.empty(B, n_out, dtype=torch.float32, device=x.device)
        out_lens = torch.empty(B, dtype=torch.int32, device=x.device) if want_lengths else None
        _lib.call("t2s_resample_batch", _lib.ptr(x), int(x.dtype == torch.float16), B, N, ldx, _lib.ptr(lens_d), *self._filter(),
                  _lib.ptr(out), n_out, n_out, _lib.ptr(out_lens), _lib.current_stream())
        return out, out_lens

    def forward(self, audio):
        """audio [N], [B, N] or [B, 1, N], float32 or float16 in HBM -> float32 of the same rank with out_length(N) samples a row"""
        x, B, N, ldx = self._rows(audio, "Resampler.forward")
        if self.up == self.down:
            return audio.detach().to(torch.float32, copy=True)
        out, _ = self._batch(x, B, N, ldx, None, False)
        return out.view(audio.shape[:-1] + (out.size(1),))

    __call__ = forward

    def resample_batch(self, audio, lengths):
        """A padded batch, e.g. Denoiser.denoise_batch's two results as returned: audio [B, T] or [B, 1, T] float32 or float16 and
        lengths [B] (a device tensor is used where it is - nothing is read back; a host tensor or a sequence is copied over).
        Returns (audio_out float32 of the same rank with out_length(T) samples a row, out_lengths int64 [B] on the device): entry
        b's first ceil(lengths[b] up / down) samples are forward(audio[b, :lengths[b]])'s bit for bit, the rest zeros; samples at and
        behind lengths[b] are never read, and lengths are clamped to [0, T] on the device."""
        what = "Resampler.resample_batch"
        if audio.dim() not in (2, 3):
            raise _lib.T2SError("%s: audio must be [B, T] or [B, 1, T], got %s" % (what, tuple(audio.shape)))
        x, B, N, ldx = self._rows(audio, what)
        try:
            lens = torch.as_tensor(lengths)
        except (TypeError, ValueError, RuntimeError) as e:
            raise _lib.T2SError("%s: lengths must be a tensor or a sequence of integers (%s)" % (what, e))
        if lens.is_floating_point() or lens.is_complex() or lens.dtype == torch.bool:
            raise _lib.T2SError("%s: lengths must be integers, got %s" % (what, lens.dtype))
        if lens.dim() != 1 or lens.numel() != B:
            raise _lib.T2SError("%s: lengths has shape %s, the batch holds %d entries" % (what, tuple(lens.shape), B))
        if lens.is_cuda:
            lens_d = lens.detach().clamp(0, N).to(torch.int32).contiguous()
        else:
            lens_d = _to_device(lens.detach().clamp(0, N).to(torch.int32).contiguous(), x.device)
        if self.up == self.down:
            return audio.detach().to(torch.float32, copy=True), lens_d.to(torch.int64)
        out, out_lens = self._batch(x, B, N, ldx, lens_d, True)
        return out.view(audio.shape[:-1] + (out.size(1),)), out_lens.to(torch.int64)


TRIM_MAX_FRAME = 8192          # the library's limit on frame_length (include/t2s_hip.h)
_KINDS = {torch.int16: 0, torch.float32: 1, torch.float16: 2}


def _float_rows(audio, lengths, what, int16_way="PcmPool.rescale_trim"):
    """audio [N], [B, N] or [B, 1, N] f32 / f16 in HBM and lengths (None: every row whole) -> (flat view over the rows, B, N,
    ldx, int64 lengths on the device clamped to [0, N]); nothing is read back"""
    _need_cuda(audio, what)
    if audio.dim() not in (1, 2, 3) or (audio.dim() == 3 and audio.size(1) != 1) or audio.numel() == 0:
        raise _lib.T2SError("%s: audio must be [N], [B, N] or [B, 1, N] and hold samples, got %s" % (what, tuple(audio.shape)))
    x = audio.detach()
    if x.dtype not in (torch.float32, torch.float16):
        raise _lib.T2SError("%s: expected float32 or float16, got %s (int16 pools go through %s)" % (what, x.dtype, int16_way))
    N = x.size(-1)
    x = x.reshape(-1, N)
    B = x.size(0)
    if B > 65535:
        raise _lib.T2SError("%s: %d rows, the most is 65535" % (what, B))
    if x.stride(1) != 1 or (B > 1 and x.stride(0) < N):
        x = x.contiguous()
    ldx = x.stride(0) if B > 1 else N
    if lengths is None:
        lens_d = torch.full((B,), N, dtype=torch.int64, device=x.device)
    else:
        try:
            lens = torch.as_tensor(lengths)
        except (TypeError, ValueError, RuntimeError) as e:
            raise _lib.T2SError("%s: lengths must be a tensor or a sequence of integers (%s)" % (what, e))
        if lens.is_floating_point() or lens.is_complex() or lens.dtype == torch.bool:
            raise _lib.T2SError("%s: lengths must be integers, got %s" % (what, lens.dtype))
        if lens.dim() != 1 or lens.numel() != B:
            raise _lib.T2SError("%s: lengths has shape %s, the batch holds %d entries" % (what, tuple(lens.shape), B))
        lens = lens.detach().to(torch.int64).clamp(0, N)
        lens_d = lens if lens.is_cuda else _to_device(lens.contiguous(), x.device)
    return torch.as_strided(x, ((B - 1) * ldx + N,), (1,)), B, N, ldx, lens_d


class Trimmer:
    """Silence trimming and peak rescaling in HBM (csrc/trim.hip): librosa.effects.trim(x, top_db, frame_length, hop_length)'s cut
    points - the first and the last frame whose RMS lies less than top_db below the loudest frame's, frames centred with
    frame_length // 2 samples of padding (`pad_mode` "reflect": librosa < 0.10, what the reference ran; "constant": zeros,
    librosa >= 0.10) - and the reference's `wav / abs(wav).max() * rescaling_max` (datasets/kss.py:68-74; utils/audio.py:14-17 with
    its 0.01 as `peak_floor`: the gain is rescaling_max / max(peak, peak_floor)).  Either half is optional: top_db=None keeps every
    sample, rescaling_max=None copies them bit for bit.  The decision is taken on the source samples with the gain inside its
    1e-10 floor, which is what trimming the rescaled floats decides (include/t2s_hip.h states the rule); a clip with a non-finite
    sample trims to nothing, and so does a clip of zeros (librosa's floor would keep that one whole).  librosa is restated, not
    imported."""

    def __init__(self, frame_length=512, hop_length=128, top_db=23, pad_mode="reflect", rescaling_max=None, peak_floor=0.0):
        T2SError = _lib.T2SError
        if int(frame_length) != frame_length or not 2 <= frame_length <= TRIM_MAX_FRAME:
            raise T2SError("Trimmer: frame_length must be an integer in [2, %d], got %r" % (TRIM_MAX_FRAME, frame_length))
        if int(hop_length) != hop_length or not 1 <= hop_length <= frame_length:
            raise T2SError("Trimmer: hop_length must be an integer in [1, frame_length], got %r" % (hop_length,))
        if pad_mode not in ("reflect", "constant"):
            raise T2SError("Trimmer: pad_mode must be 'reflect' or 'constant', got %r" % (pad_mode,))
        for name, v, positive in (("top_db", top_db, False), ("rescaling_max", rescaling_max, True), ("peak_floor", peak_floor, False)):
            if v is None and name != "peak_floor":
                continue
            if v is None or not np.isfinite(v) or v < 0 or (positive and v == 0):
                raise T2SError("Trimmer: %s must be finite and %s, got %r" % (name, "positive" if positive else "not negative", v))
        self.frame_length, self.hop_length, self.pad_mode = int(frame_length), int(hop_length), pad_mode
        self.top_db = None if top_db is None else float(top_db)
        self.rescaling_max = None if rescaling_max is None else float(rescaling_max)
        self.peak_floor = float(peak_floor)

    @property
    def pad(self):
        return self.frame_length // 2

    def n_frames(self, n):
        """frames of a clip of n samples: 1 + (n + 2 pad - frame_length) // hop_length"""
        return 1 + (int(n) + 2 * self.pad - self.frame_length) // self.hop_length

    def _stats_bounds(self, src, table3, n_rows, max_count, energy_len, stats=None):
        """The energy pass and (with top_db) the bounds pass over `table3` (device int64 [n_rows, 3]: src_start, src_count,
        energy_start) of the flat device tensor `src` -> (stats [n_rows, 2] float64, bounds [n_rows, 2] int64 or None)."""
        p, dev = _lib.ptr, src.device
        if stats is None:
            stats = torch.empty(n_rows, 2, dtype=torch.float64, device=dev)
        mode = 0 if self.pad_mode == "reflect" else 1
        max_frames = max(1, self.n_frames(max_count))
        energy = torch.empty(int(energy_len), dtype=torch.float64, device=dev) if self.top_db is not None else None
        frames = (self.frame_length, self.hop_length, mode, max_frames)
        _lib.call("t2s_trim_energy", p(src), _KINDS[src.dtype], src.numel(), p(table3), n_rows, *frames, p(energy),
                  0 if energy is None else energy.numel(), p(stats), _lib.current_stream())
        if energy is None:
            return stats, None
        bounds = torch.empty(n_rows, 2, dtype=torch.int64, device=dev)
        _lib.call("t2s_trim_bounds", p(table3), n_rows, _KINDS[src.dtype], src.numel(), *frames, p(energy), energy.numel(), p(stats),
                  self.top_db, int(self.rescaling_max is not None), self.rescaling_max or 0.0, self.peak_floor, p(bounds),
                  _lib.current_stream())
        return stats, bounds

    def _gather(self, src, table4, n_rows, bounds, stats, dst, max_out, out_lengths=None):
        p = _lib.ptr
        rescale = self.rescaling_max is not None
        _lib.call("t2s_trim_gather", p(src), _KINDS[src.dtype], src.numel(), p(table4), n_rows, p(bounds), p(stats if rescale else None),
                  self.rescaling_max or 0.0, self.peak_floor, p(dst), _KINDS[dst.dtype], dst.numel(), int(max_out), p(out_lengths),
                  _lib.current_stream())

    def _rows(self, audio, lengths, what):
        return _float_rows(audio, lengths, what)

    def _batch_bounds(self, flat, B, N, ldx, lens_d):
        """(stats, bounds, row index) of a padded batch; the tables are built on the device"""
        rows = torch.arange(B, dtype=torch.int64, device=flat.device)
        per_row = max(1, self.n_frames(N))
        table3 = torch.stack([rows * ldx, lens_d, rows * per_row], 1).contiguous()
        stats, bounds = self._stats_bounds(flat, table3, B, N, B * per_row)
        return stats, bounds, rows

    def bounds_batch(self, audio, lengths):
        """(start, end), int64 [B] on the device: entry b keeps audio[b, start[b]:end[b]]; (0, 0) where nothing is loud.  Without
        top_db: (0, lengths).  Nothing is read back."""
        flat, B, N, ldx, lens_d = self._rows(audio, lengths, "Trimmer.bounds_batch")
        if self.top_db is None:
            return torch.zeros_like(lens_d), lens_d.clone()
        _, bounds, _ = self._batch_bounds(flat, B, N, ldx, lens_d)
        return bounds[:, 0].contiguous(), bounds[:, 1].contiguous()

    def _trim(self, audio, lengths, what):
        flat, B, N, ldx, lens_d = self._rows(audio, lengths, what)
        stats = bounds = None
        rows = torch.arange(B, dtype=torch.int64, device=flat.device)
        if self.top_db is not None or self.rescaling_max is not None:
            stats, bounds, rows = self._batch_bounds(flat, B, N, ldx, lens_d)
        out = torch.empty(B, N, dtype=torch.float32, device=flat.device)
        out_lens = torch.empty(B, dtype=torch.int32, device=flat.device)
        table4 = torch.stack([rows * ldx, lens_d, rows * N, torch.full_like(rows, N)], 1).contiguous()
        self._gather(flat, table4, B, bounds, stats, out.view(-1), N, out_lens)
        return out, out_lens

    def forward(self, audio):
        """One clip: audio [T], [1, T] or [1, 1, T], float32 or float16 in HBM -> the kept samples, rescaled where rescaling_max is
        set, float32 of the same rank.  One read-back, of the kept length (none without top_db)."""
        what = "Trimmer.forward"
        if torch.is_tensor(audio) and (audio.dim() not in (1, 2, 3) or audio.numel() != audio.size(-1)):
            raise _lib.T2SError("%s: audio must be one clip, [T], [1, T] or [1, 1, T], got %s" % (what, tuple(audio.shape)))
        out, out_lens = self._trim(audio, None, what)
        keep = audio.size(-1) if self.top_db is None else int(out_lens[0])
        return out[0, :keep].view(audio.shape[:-1] + (keep,))

    __call__ = forward

    def trim_batch(self, audio, lengths):
        """A padded batch, e.g. Denoiser.denoise_batch's two results as returned: audio [B, T] or [B, 1, T] float32 or float16 and
        lengths [B] (a device tensor is used where it is; a host tensor or a sequence is copied over).  Returns (audio_out float32
        of audio's shape, out_lengths int32 [B] on the device): entry b's first out_lengths[b] samples are
        forward(audio[b, :lengths[b]])'s bit for bit, moved to column 0, the rest of its row zeros; an entry in which nothing is
        loud gets length 0.  Samples at and behind lengths[b] are never read, lengths are clamped to [0, T] on the device, and
        nothing is read back."""
        what = "Trimmer.trim_batch"
        if not torch.is_tensor(audio) or audio.dim() not in (2, 3):
            raise _lib.T2SError("%s: audio must be [B, T] or [B, 1, T], got %s" % (what, tuple(getattr(audio, "shape", ()))))
        out, out_lens = self._trim(audio, lengths, what)
        return out.view(audio.shape), out_lens


LOUD_MIN_RATE, LOUD_MAX_RATE = 4000, 384000    # the library's limits on the hop, as rates (include/t2s_hip.h)
LOUD_GATE_ABS = 10.0 ** ((-70.0 + 0.691) / 10.0)       # BS.1770's absolute gate, as a mean square
LOUD_FLAG_SHORT, LOUD_FLAG_SILENT, LOUD_FLAG_PEAK, LOUD_FLAG_NONFINITE = 1, 2, 4, 8

LoudnessReport = collections.namedtuple("LoudnessReport", "ms lufs peak gain blocks flags")


def loudness_coefficients(sampling_rate):
    """BS.1770's K-weighting at any rate, float64: ((b, a) of the shelf, (b, a) of the high-pass), a[0] = 1.  The analogue
    prototypes behind the standard's 48 kHz table, bilinear-transformed: at 48 000 Hz these give the printed table to 1e-15."""
    fs = float(sampling_rate)

    def stage(f0, Q, shelf_db):
        K = np.tan(np.pi * f0 / fs)
        a0 = 1.0 + K / Q + K * K
        a = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
        if shelf_db is None:
            return np.array([1.0, -2.0, 1.0]), a
        Vh = 10.0 ** (shelf_db / 20.0)
        Vb = Vh ** 0.4996667741545416
        return np.array([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0]), a

    return stage(1681.974450955533, 0.7071752369554196, 3.999843853973347), stage(38.13547087602444, 0.5003270373238773, None)


def loudness_hop(sampling_rate):
    """samples of BS.1770's 100 ms hop at an integer rate: floor(fs / 10 + 1 / 2)"""
    return (2 * int(sampling_rate) + 10) // 20


def loudness_table(sampling_rate, segment, lanes=256):
    """t2s_loud_measure's `coef` (include/t2s_hip.h states the layout), float64 [160]: both biquads, then the zero-input map of
    `segment` samples on the cascade's state raised to 2^k, k = 0 .. log2(lanes) - 1, then that of a tile of lanes segments."""
    (b1, a1), (b2, a2) = loudness_coefficients(sampling_rate)
    # one sample with x = 0: y1 = s0; s0' = -a1[1] y1 + s1; s1' = -a1[2] y1; y2 = b2[0] y1 + s2; s2' = b2[1] y1 - a2[1] y2 + s3; ...
    M = np.zeros((4, 4))
    M[0] = [-a1[1], 1.0, 0.0, 0.0]
    M[1] = [-a1[2], 0.0, 0.0, 0.0]
    M[2] = [b2[1] - a2[1] * b2[0], 0.0, -a2[1], 1.0]
    M[3] = [b2[2] - a2[2] * b2[0], 0.0, -a2[2], 0.0]
    steps = int(lanes).bit_length() - 1
    assert 1 << steps == lanes and steps == 8
    out = np.zeros(16 + 16 * steps + 16)
    out[0:5] = [b1[0], b1[1], b1[2], a1[1], a1[2]]
    out[5:10] = [b2[0], b2[1], b2[2], a2[1], a2[2]]
    P = np.linalg.matrix_power(M, int(segment))
    for k in range(steps):
        out[16 + 16 * k:32 + 16 * k] = P.reshape(-1)
        P = P @ P
    out[16 + 16 * steps:] = P.reshape(-1)
    return out


class Loudness:
    """Programme loudness in HBM (csrc/loudness.hip): ITU-R BS.1770-4 / EBU R128 gated loudness of every row - K-weighting, 400 ms
    blocks on a 100 ms hop, the absolute gate at -70 LUFS and the relative one 10 LU below the gated mean - and the gain that brings
    the row to `target_lufs` (-23: EBU R128's programme level, a convention), limited so that no sample exceeds `peak_limit` (a
    sample peak, not a true peak; None: no limit).  include/t2s_hip.h states the arithmetic.  A row shorter than 0.4 s, one with
    nothing above -70 LUFS and one with a non-finite sample are flagged (LOUD_FLAG_*) and left as they are (gain 1).  Mono; nothing
    is read back, everything runs on the caller's current stream, and a row's result does not depend on the batch around it."""

    def __init__(self, sampling_rate, target_lufs=-23.0, peak_limit=None, device="cuda"):
        T2SError = _lib.T2SError
        try:
            whole = not isinstance(sampling_rate, bool) and int(sampling_rate) == sampling_rate
        except (TypeError, ValueError, OverflowError):
            whole = False
        if not whole or not LOUD_MIN_RATE <= sampling_rate <= LOUD_MAX_RATE:
            raise T2SError("Loudness: sampling_rate must be an integer in [%d, %d], got %r" % (LOUD_MIN_RATE, LOUD_MAX_RATE, sampling_rate))
        if not isinstance(target_lufs, (int, float, np.floating, np.integer)) or not np.isfinite(target_lufs):
            raise T2SError("Loudness: target_lufs must be finite, got %r" % (target_lufs,))
        if peak_limit is not None and (not isinstance(peak_limit, (int, float, np.floating, np.integer)) or not np.isfinite(peak_limit)
                                       or peak_limit <= 0):
            raise T2SError("Loudness: peak_limit must be None or finite and positive, got %r" % (peak_limit,))
        dev = torch.device(device)
        if dev.type != "cuda":
            raise T2SError("Loudness: the filter table lives in HBM (cuda); there is no CPU path")
        self.sampling_rate, self.hop = int(sampling_rate), loudness_hop(sampling_rate)
        self.target_lufs = float(target_lufs)
        self.target_T = 10.0 ** ((self.target_lufs + 0.691) / 10.0)
        self.peak_limit = None if peak_limit is None else float(peak_limit)
        self.device = dev
        self._coef = None           # uploaded by the first call (1.3 KB, a blocking copy): constructing needs no device

    def _table(self, dev):
        if self._coef is None or self._coef.device != dev:
            lib = _lib.load()
            # (blocking, so that the table is whole before any stream can read it)
            self._coef = torch.from_numpy(loudness_table(self.sampling_rate, lib.t2s_loud_segment(),
                                                         lib.t2s_loud_tile() // lib.t2s_loud_segment())).to(dev)
        return self._coef

    def _measure(self, src, table2, n_rows, max_count, stats=None, counts=None):
        """t2s_loud_measure over `table2` (device int64 [n_rows, 2]: src_start, src_count) of the flat device tensor `src`
        -> (stats float64 [n_rows, 4], counts int32 [n_rows, 4])"""
        p, dev = _lib.ptr, src.device
        max_count = max(1, int(max_count))
        if max_count > 2 ** 31 - 1:
            raise _lib.T2SError("Loudness: a row of %d samples, the most is 2^31 - 1" % max_count)
        if stats is None:
            stats = torch.empty(n_rows, 4, dtype=torch.float64, device=dev)
            counts = torch.empty(n_rows, 4, dtype=torch.int32, device=dev)
        need = _lib.load().t2s_loud_scratch(n_rows, max_count)
        scratch = torch.empty(need, dtype=torch.float64, device=dev)
        _lib.call("t2s_loud_measure", p(src), _KINDS[src.dtype], src.numel(), p(table2), n_rows, max_count, self.hop, p(self._table(dev)),
                  p(scratch), need, LOUD_GATE_ABS, self.target_T, self.peak_limit or 0.0, p(stats), p(counts), _lib.current_stream())
        return stats, counts

    @staticmethod
    def _apply(src, table4, n_rows, stats, dst, max_out):
        p = _lib.ptr
        _lib.call("t2s_loud_apply", p(src), _KINDS[src.dtype], src.numel(), p(table4), n_rows, p(stats), p(dst), _KINDS[dst.dtype],
                  dst.numel(), max(1, int(max_out)), None, _lib.current_stream())

    @staticmethod
    def _report(stats, counts):
        return LoudnessReport(stats[:, 0], stats[:, 1], stats[:, 2], stats[:, 3], counts[:, 0], counts[:, 3])

    def _batch(self, audio, lengths, what):
        flat, B, N, ldx, lens_d = _float_rows(audio, lengths, what, "PcmPool.normalize_loudness")
        rows = torch.arange(B, dtype=torch.int64, device=flat.device)
        stats, counts = self._measure(flat, torch.stack([rows * ldx, lens_d], 1).contiguous(), B, N)
        return flat, B, N, ldx, lens_d, rows, stats, counts

    def measure_batch(self, audio, lengths=None):
        """audio [N], [B, N] or [B, 1, N] float32 or float16 in HBM (strided rows are taken where they are) and lengths [B] (the
        int32 device tensor infer_batch / trim_batch return is used where it is; None: whole rows) -> LoudnessReport(ms, lufs, peak,
        gain float64 [B], blocks, flags int32 [B]), all on the device.  Samples at and behind lengths[b] are never read."""
        return self._report(*self._batch(audio, lengths, "Loudness.measure_batch")[-2:])

    def normalize_batch(self, audio, lengths=None):
        """-> (audio float32 of audio's shape, lengths as given): entry b's first lengths[b] samples times its gain - forward(
        audio[b, :lengths[b]])'s bit for bit - and zeros behind them.  A flagged row is copied.  Nothing is read back."""
        what = "Loudness.normalize_batch"
        flat, B, N, ldx, lens_d, rows, stats, _ = self._batch(audio, lengths, what)
        out = torch.empty(B, N, dtype=torch.float32, device=flat.device)
        table4 = torch.stack([rows * ldx, lens_d, rows * N, torch.full_like(rows, N)], 1).contiguous()
        self._apply(flat, table4, B, stats, out.view(-1), N)
        return out.view(audio.shape), lengths

    def forward(self, audio):
        """One clip [N] / [1, N], or whole rows [B, N] / [B, 1, N], float32 or float16 in HBM -> float32 of the same shape"""
        return self.normalize_batch(audio, None)[0]

    __call__ = forward

    def normalize_limit_batch(self, audio, lengths, limiter):
        """normalize_batch with `limiter` (a Limiter at this rate) in place of a lowered row gain: measure_batch, then
        limiter.limit_batch(audio, lengths, gain=report.gain) - the loudness gain and the limiter in one pass over the samples, no
        buffer in between, nothing read back.  A row keeps its loudness gain and only the surroundings of its peaks are taken down
        to the limiter's ceiling.  Construct this Loudness with peak_limit=None for that; a peak_limit still lowers the row gain
        first.  -> (audio float32 of audio's shape, lengths as given)"""
        if not isinstance(limiter, Limiter):
            raise _lib.T2SError("Loudness.normalize_limit_batch: limiter must be an audio.Limiter, got a %s" % type(limiter).__name__)
        if limiter.sampling_rate != self.sampling_rate:
            raise _lib.T2SError("Loudness.normalize_limit_batch: the limiter is built for %d Hz, this Loudness for %d"
                                % (limiter.sampling_rate, self.sampling_rate))
        report = self.measure_batch(audio, lengths)
        return limiter.limit_batch(audio, lengths, gain=report.gain)


LIMIT_MAX_LOOKAHEAD = 1024     # the library's limits (include/t2s_hip.h)
LIMIT_MAX_HALF_WIDTH = 32
LIMIT_FLAG_LIMITED, LIMIT_FLAG_NONFINITE = 1, 8

LimiterReport = collections.namedtuple("LimiterReport", "true_peak sample_peak min_gain limited flags")


def limiter_window(lookahead):
    """t2s_limit_measure's `w`, float64 [2 L + 1]: w[k] = 1/2 + 1/2 cos(pi k / (L + 1)) for k = -L .. L, normalised to sum 1 - and
    the centre tap raised by the few ulps it may take for the sum in ASCENDING order, as the kernel adds it, to be no less than 1:
    the smoothed gain is then exactly 1 wherever every minimum in reach is 1, which is what lets an untouched stretch keep its
    bits."""
    L = int(lookahead)
    w = 0.5 + 0.5 * np.cos(np.pi * np.arange(-L, L + 1, dtype=np.float64) / (L + 1))
    w = w / w.sum()

    def asc():
        acc = 0.0
        for v in w:
            acc += float(v)
        return acc

    while asc() < 1.0:
        w[L] += max(1.0 - asc(), np.spacing(w[L]))
    return w


def _real(v):
    return isinstance(v, (int, float, np.floating, np.integer)) and not isinstance(v, bool) and np.isfinite(v)


class Limiter:
    """A true-peak meter and look-ahead limiter in HBM (csrc/limiter.hip), the last stage of a delivery chain: resample first,
    limit last at the delivery rate, then to_pcm16.  include/t2s_hip.h states the arithmetic: the row's envelope `oversample`
    times oversampled with resample_filter(1, oversample, half_width, beta) - scipy.signal.resample_poly's own filter, the
    project's interpolator, not BS.1770 Annex 2's printed 48-tap table, which is one admissible choice - the gain ceiling / peak
    each sample needs, its minimum over +-lookahead samples, that smoothed by a normalised Hann window, and the row times the
    result.  `ceiling` is 10^(ceiling_db / 20) rounded to float32; `lookahead` = round(sampling_rate lookahead_ms / 1000)
    samples; an output sample depends on the input over +-`reach` = 2 lookahead + half_width samples only.  GUARANTEED: no output
    sample exceeds `ceiling` in magnitude, exactly.  NOT guaranteed: the output's true peak - a moving gain changes the values
    between the samples; at oversample=4 and the default look-ahead it came to about 1 + 2e-5 of the ceiling and less
    (profiles/limiter_tests.md).  Mono; nothing is read back, everything runs on the caller's current stream, and a row's result
    does not depend on the batch around it.  A row with a non-finite sample is flagged (LIMIT_FLAG_NONFINITE) and copied."""

    def __init__(self, sampling_rate, ceiling_db=-1.0, lookahead_ms=1.5, oversample=4, half_width=10, beta=5.0, device="cuda"):
        T2SError = _lib.T2SError
        try:
            whole = not isinstance(sampling_rate, bool) and int(sampling_rate) == sampling_rate
        except (TypeError, ValueError, OverflowError):
            whole = False
        if not whole or sampling_rate < 1:
            raise T2SError("Limiter: sampling_rate must be a positive integer, got %r" % (sampling_rate,))
        if not _real(ceiling_db) or ceiling_db > 0:
            raise T2SError("Limiter: ceiling_db must be finite and at most 0 (dB relative to full scale), got %r" % (ceiling_db,))
        if not _real(lookahead_ms) or lookahead_ms < 0:
            raise T2SError("Limiter: lookahead_ms must be finite and not negative, got %r" % (lookahead_ms,))
        lookahead = int(round(int(sampling_rate) * float(lookahead_ms) / 1000.0))
        if lookahead > LIMIT_MAX_LOOKAHEAD:
            raise T2SError("Limiter: lookahead_ms = %r is %d samples at %d Hz, the most is %d"
                           % (lookahead_ms, lookahead, sampling_rate, LIMIT_MAX_LOOKAHEAD))
        if isinstance(oversample, bool) or oversample not in (1, 2, 4):
            raise T2SError("Limiter: oversample must be 1, 2 or 4, got %r" % (oversample,))
        if isinstance(half_width, bool) or not isinstance(half_width, (int, np.integer)) or not 1 <= half_width <= LIMIT_MAX_HALF_WIDTH:
            raise T2SError("Limiter: half_width must be an integer in [1, %d], got %r" % (LIMIT_MAX_HALF_WIDTH, half_width))
        if not _real(beta) or beta < 0:
            raise T2SError("Limiter: beta must be finite and not negative, got %r" % (beta,))
        ceiling = float(np.float32(10.0 ** (float(ceiling_db) / 20.0)))
        if not ceiling > 0.0:
            raise T2SError("Limiter: ceiling_db = %r gives a ceiling of 0 in float32" % (ceiling_db,))
        dev = torch.device(device)
        if dev.type != "cuda":
            raise T2SError("Limiter: the filter and the window live in HBM (cuda); there is no CPU path")
        self.sampling_rate = int(sampling_rate)
        self.ceiling_db, self.ceiling = float(ceiling_db), ceiling
        self.lookahead, self.oversample, self.half_width, self.beta = lookahead, int(oversample), int(half_width), float(beta)
        self.reach = 2 * lookahead + self.half_width
        self.n_taps = 2 * self.half_width * self.oversample + 1
        self.device = dev
        self._tables = None         # uploaded by the first call (a blocking copy): constructing needs no device

    def _hw(self, dev):
        """(h, w) on the device: the interpolation filter and the smoothing window, one upload"""
        if self._tables is None or self._tables.device != dev:
            h = resample_filter(1, self.oversample, self.half_width, self.beta)[2]
            assert h.size == self.n_taps
            # (blocking, so that the tables are whole before any stream can read them)
            self._tables = torch.from_numpy(np.concatenate([h, limiter_window(self.lookahead)])).to(dev)
        return self._tables[:self.n_taps], self._tables[self.n_taps:]

    def _params(self, dev):
        h, w = self._hw(dev)
        return _lib.ptr(h), self.n_taps, self.oversample, self.half_width, _lib.ptr(w), self.lookahead, self.ceiling

    def _measure(self, src, table2, n_rows, max_count, gains=None, stats=None, counts=None):
        """t2s_limit_measure over `table2` (device int64 [n_rows, 2]: src_start, src_count) of the flat device tensor `src`
        -> (stats float64 [n_rows, 4], counts int32 [n_rows, 2])"""
        p, dev = _lib.ptr, src.device
        max_count = max(1, int(max_count))
        if max_count > 2 ** 31 - 1:
            raise _lib.T2SError("Limiter: a row of %d samples, the most is 2^31 - 1" % max_count)
        if stats is None:
            stats = torch.empty(n_rows, 4, dtype=torch.float64, device=dev)
            counts = torch.empty(n_rows, 2, dtype=torch.int32, device=dev)
        need = _lib.load().t2s_limit_scratch(n_rows, max_count)
        scratch = torch.empty(need, dtype=torch.float64, device=dev)
        _lib.call("t2s_limit_measure", p(src), _KINDS[src.dtype], src.numel(), p(table2), n_rows, max_count, p(gains),
                  *self._params(dev), p(scratch), need, p(stats), p(counts), _lib.current_stream())
        return stats, counts

    def _apply(self, src, table4, n_rows, gains, counts, dst, max_out):
        p = _lib.ptr
        _lib.call("t2s_limit_apply", p(src), _KINDS[src.dtype], src.numel(), p(table4), n_rows, p(gains), *self._params(src.device),
                  p(counts), p(dst), _KINDS[dst.dtype], dst.numel(), max(1, int(max_out)), None, _lib.current_stream())

    @staticmethod
    def _report(stats, counts):
        return LimiterReport(stats[:, 0], stats[:, 1], stats[:, 2], counts[:, 0], counts[:, 1])

    @staticmethod
    def _check(audio, lengths, gain, what):
        """what needs no device to refuse: the shapes and types of audio, lengths and gain (the messages of _float_rows)"""
        T2SError = _lib.T2SError
        if not torch.is_tensor(audio):
            raise T2SError("%s: audio must be a tensor, got a %s" % (what, type(audio).__name__))
        if audio.dim() not in (1, 2, 3) or (audio.dim() == 3 and audio.size(1) != 1) or audio.numel() == 0:
            raise T2SError("%s: audio must be [N], [B, N] or [B, 1, N] and hold samples, got %s" % (what, tuple(audio.shape)))
        if audio.dtype not in (torch.float32, torch.float16):
            raise T2SError("%s: expected float32 or float16, got %s (int16 pools go through PcmPool.limit)" % (what, audio.dtype))
        B = audio.numel() // audio.size(-1)
        if B > 65535:
            raise T2SError("%s: %d rows, the most is 65535" % (what, B))
        if lengths is not None:
            try:
                lens = torch.as_tensor(lengths)
            except (TypeError, ValueError, RuntimeError) as e:
                raise T2SError("%s: lengths must be a tensor or a sequence of integers (%s)" % (what, e))
            if lens.is_floating_point() or lens.is_complex() or lens.dtype == torch.bool:
                raise T2SError("%s: lengths must be integers, got %s" % (what, lens.dtype))
            if lens.dim() != 1 or lens.numel() != B:
                raise T2SError("%s: lengths has shape %s, the batch holds %d entries" % (what, tuple(lens.shape), B))
        if gain is not None:
            if not torch.is_tensor(gain) or gain.dtype != torch.float64:
                raise T2SError("%s: gain must be None or a float64 tensor in HBM (e.g. LoudnessReport.gain), got %s"
                               % (what, gain.dtype if torch.is_tensor(gain) else "a %s" % type(gain).__name__))
            if gain.dim() != 1 or gain.numel() != B:
                raise T2SError("%s: gain has shape %s, the batch holds %d entries" % (what, tuple(gain.shape), B))
            if gain.device != audio.device:
                raise T2SError("%s: gain is on %s, audio on %s" % (what, gain.device, audio.device))

    def _batch(self, audio, lengths, gain, what):
        self._check(audio, lengths, gain, what)
        flat, B, N, ldx, lens_d = _float_rows(audio, lengths, what, "PcmPool.limit")
        gains = None if gain is None else gain.detach().contiguous()    # (a strided view such as LoudnessReport.gain: packed here)
        rows = torch.arange(B, dtype=torch.int64, device=flat.device)
        stats, counts = self._measure(flat, torch.stack([rows * ldx, lens_d], 1).contiguous(), B, N, gains)
        return flat, B, N, ldx, lens_d, rows, gains, stats, counts

    def true_peak_batch(self, audio, lengths=None, gain=None):
        """audio [N], [B, N] or [B, 1, N] float32 or float16 in HBM (strided rows are read where they are), lengths [B] (an int32
        or int64 device tensor is used where it is, a host sequence is copied over; None: whole rows) and gain (None, or a float64
        device tensor [B] the rows are multiplied by first) -> LimiterReport(true_peak, sample_peak, min_gain float64 [B],
        limited, flags int32 [B]), all on the device: the peaks of the INPUT times its gain, the smallest gain limit_batch would
        apply and the number of samples over the ceiling.  Samples at and behind lengths[b] are never read."""
        return self._report(*self._batch(audio, lengths, gain, "Limiter.true_peak_batch")[-2:])

    def limit_batch(self, audio, lengths=None, gain=None):
        """-> (audio float32 of audio's shape, lengths as given): entry b's first lengths[b] samples times its gain, limited -
        forward(audio[b, :lengths[b]])'s bit for bit - and zeros behind them.  A row with nothing over the ceiling and no gain is
        copied bit for bit.  Nothing is read back."""
        what = "Limiter.limit_batch"
        flat, B, N, ldx, lens_d, rows, gains, _, counts = self._batch(audio, lengths, gain, what)
        out = torch.empty(B, N, dtype=torch.float32, device=flat.device)
        table4 = torch.stack([rows * ldx, lens_d, rows * N, torch.full_like(rows, N)], 1).contiguous()
        self._apply(flat, table4, B, gains, counts, out.view(-1), N)
        return out.view(audio.shape), lengths

    def forward(self, audio):
        """One clip [N] / [1, N], or whole rows [B, N] / [B, 1, N], float32 or float16 in HBM -> float32 of the same shape"""
        return self.limit_batch(audio, None)[0]

    __call__ = forward


SOS_MAX_SECTIONS = 8           # the library's limits and geometry (include/t2s_hip.h)
SOS_TABLE_DOUBLES = 552

FilterReport = collections.namedtuple("FilterReport", "nonfinite clipped")


def _check_sos(sos, what="SosFilter"):
    """`sos` as a validated float64 [n, 6] array (scipy.signal.sosfilt's layout, a0 = 1, every pole inside the unit circle);
    anything else raises T2SError naming the offending value.  Host only."""
    T2SError = _lib.T2SError
    try:
        s = np.array(sos, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise T2SError("%s: sos must be an array [n, 6] of numbers (%s)" % (what, e))
    if s.ndim != 2 or s.shape[1] != 6:
        raise T2SError("%s: sos must have shape [n, 6] (b0 b1 b2 a0 a1 a2), got %s" % (what, tuple(s.shape)))
    n = s.shape[0]
    if not 1 <= n <= SOS_MAX_SECTIONS:
        raise T2SError("%s: %d sections, from 1 to %d" % (what, n, SOS_MAX_SECTIONS))
    for j in range(n):
        if not np.all(np.isfinite(s[j])):
            raise T2SError("%s: section %d holds a coefficient that is not finite: %s" % (what, j, s[j].tolist()))
        if s[j, 3] != 1.0:
            raise T2SError("%s: section %d has a0 = %r, it must be exactly 1 (normalise the section)" % (what, j, float(s[j, 3])))
        radius = float(np.max(np.abs(np.roots(s[j, 3:]))))
        if not radius < 1.0:
            raise T2SError("%s: section %d has a pole of radius %.17g, it must lie inside the unit circle" % (what, j, radius))
    return s


def _sos_zero_input(sos, steps, marks):
    """The cascade `sos` [n, 6] run for `steps` samples with zero input from each unit state of its 2n-vector (s1, s2 of section 0,
    s1, s2 of section 1, ...), in float64, one column per unit state: {m: the 2n x 2n map after m samples} for m in marks."""
    n = sos.shape[0]
    st = np.eye(2 * n)                                          # st[2 j], st[2 j + 1]: s1, s2 of section j, one column per start
    out = {}
    for t in range(1, steps + 1):
        x = np.zeros(2 * n)
        for j in range(n):
            b0, b1, b2, _, a1, a2 = sos[j]
            y = b0 * x + st[2 * j]
            st[2 * j] = (b1 * x + st[2 * j + 1]) - a1 * y
            st[2 * j + 1] = b2 * x - a2 * y
            x = y
        if t in marks:
            out[t] = st.copy()
    return out


def sos_table(sos, segment, lanes=256):
    """t2s_sos_filter's `tab` (include/t2s_hip.h states the layout), float64 [552]: the sections' coefficients, every section's 2 x 2
    zero-input map over segment 2^k samples, k = 0 .. log2(lanes) - 1, and the cascade's 2n x 2n map over a tile of `lanes`
    segments - each formed by running the recurrence itself on unit states with zero input, so the kernel, the restatement in
    tests/filter_ref.py and this table agree on the numbers."""
    s = _check_sos(sos, "sos_table")
    n, segment = s.shape[0], int(segment)
    steps = int(lanes).bit_length() - 1
    assert 1 << steps == lanes and steps == 8 and segment >= 1
    out = np.zeros(SOS_TABLE_DOUBLES)
    marks = [segment << k for k in range(steps)]
    for j in range(n):
        out[5 * j:5 * j + 5] = [s[j, 0], s[j, 1], s[j, 2], s[j, 4], s[j, 5]]
        maps = _sos_zero_input(s[j:j + 1], marks[-1], set(marks))
        for k, m in enumerate(marks):
            out[40 + 32 * j + 4 * k:44 + 32 * j + 4 * k] = maps[m].reshape(-1)
    tile = segment * lanes
    out[296:296 + 4 * n * n] = _sos_zero_input(s, tile, {tile})[tile].reshape(-1)
    return out


def sos_preemphasis(k=0.97):
    """The reference's preemphasis (utils/audio.py:24-27), scipy.signal.lfilter([1, -k], [1], x), as one section: float64 [1, 6]"""
    if not _real(k):
        raise _lib.T2SError("sos_preemphasis: k must be a finite number, got %r" % (k,))
    return np.array([[1.0, -float(k), 0.0, 1.0, 0.0, 0.0]])


def sos_deemphasis(k=0.97):
    """The reference's inv_preemphasis (utils/audio.py:30-33), scipy.signal.lfilter([1], [1, -k], x), as one section"""
    if not _real(k) or not abs(k) < 1.0:
        raise _lib.T2SError("sos_deemphasis: k must be a number inside (-1, 1) (the pole), got %r" % (k,))
    return np.array([[1.0, 0.0, 0.0, 1.0, -float(k), 0.0]])


def sos_butter(order, cutoff_hz, kind, sampling_rate):
    """A Butterworth design as sections, scipy.signal.butter(order, cutoff_hz, kind, fs=sampling_rate, output="sos"): float64
    [n, 6].  kind "highpass" or "lowpass" with one cutoff, "bandpass" with (low, high); a band-pass of order N has 2N poles."""
    from scipy.signal import butter
    T2SError = _lib.T2SError
    what = "sos_butter"
    if kind not in ("highpass", "lowpass", "bandpass"):
        raise T2SError("%s: kind must be 'highpass', 'lowpass' or 'bandpass', got %r" % (what, kind))
    if isinstance(order, bool) or not isinstance(order, (int, np.integer)) or order < 1:
        raise T2SError("%s: order must be a positive integer, got %r" % (what, order))
    if not _real(sampling_rate) or sampling_rate <= 0:
        raise T2SError("%s: sampling_rate must be a positive number, got %r" % (what, sampling_rate))
    cut = [cutoff_hz] if _real(cutoff_hz) else (list(cutoff_hz) if isinstance(cutoff_hz, (list, tuple, np.ndarray)) else None)
    if cut is None or len(cut) != (2 if kind == "bandpass" else 1) or not all(_real(c) and 0 < c < sampling_rate / 2 for c in cut) \
            or (len(cut) == 2 and not cut[0] < cut[1]):
        raise T2SError("%s: a %s needs %s inside (0, %g) Hz, got %r"
                       % (what, kind, "(low, high) cutoffs, low < high," if kind == "bandpass" else "one cutoff", sampling_rate / 2,
                          cutoff_hz))
    sections = int(order) if kind == "bandpass" else -(-int(order) // 2)
    if sections > SOS_MAX_SECTIONS:
        raise T2SError("%s: order %d as a %s is %d sections, the most is %d" % (what, order, kind, sections, SOS_MAX_SECTIONS))
    return np.ascontiguousarray(butter(int(order), cut if len(cut) == 2 else cut[0], kind, fs=float(sampling_rate), output="sos"),
                                dtype=np.float64)


class SosFilter:
    """An IIR filter in HBM (csrc/sosfilt.hip): a cascade of second-order sections, `sos` float64 [n, 6] in scipy.signal.sosfilt's
    layout (1 <= n <= 8, a0 = 1, every pole inside the unit circle: anything else raises T2SError here, on the host, before
    anything is uploaded).  include/t2s_hip.h states the arithmetic: every section in double from a zero state at the row's first
    sample, a sample that is not finite entering as +0 and counted.  The recursion runs in parallel along the row, so the result
    is scipy's to a rounding-reordering error that profiles/filter_tests.md records, not bit for bit - but a row's bits are the same
    alone, in any batch or pool, and cut into the pieces of a stream (stream()).  `sampling_rate` (optional) names the rate the design
    is for: a pool or a DeliveryStream at another rate then refuses it.  Mono; nothing is read back; every launch goes to the
    caller's current stream."""

    def __init__(self, sos, sampling_rate=None, device="cuda"):
        self.sos = _check_sos(sos, "SosFilter")
        if sampling_rate is not None and (not _real(sampling_rate) or sampling_rate <= 0):
            raise _lib.T2SError("SosFilter: sampling_rate must be None or a positive number, got %r" % (sampling_rate,))
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.T2SError("SosFilter: the filter table lives in HBM (cuda); there is no CPU path")
        self.n_sections = int(self.sos.shape[0])
        self.sampling_rate = sampling_rate
        self.device = dev
        self._tab_host = self._tab_dev = None       # uploaded by the first call (4.4 KB, a blocking copy): constructing needs no device

    def table(self):
        """The host table (sos_table at the library's segment and tile), float64 [552]"""
        if self._tab_host is None:
            lib = _lib.load()
            self._tab_host = sos_table(self.sos, lib.t2s_sos_segment(), lib.t2s_sos_tile() // lib.t2s_sos_segment())
        return self._tab_host

    def _tab(self, dev):
        if self._tab_dev is None or self._tab_dev.device != dev:
            # (blocking, so that the table is whole before any stream can read it)
            self._tab_dev = torch.from_numpy(self.table()).to(dev)
        return self._tab_dev

    def _filter(self, src, table4, n_rows, max_count, gains, dst, max_out, counts=None):
        """t2s_sos_filter over `table4` (device int64 [n_rows, 4]) of the flat device tensor `src` into the flat `dst` -> counts
        int32 [n_rows, 2] (nonfinite, clipped)"""
        p, dev = _lib.ptr, src.device
        max_count = max(1, int(max_count))
        if max_count > 2 ** 31 - 1:
            raise _lib.T2SError("SosFilter: a row of %d samples, the most is 2^31 - 1" % max_count)
        if counts is None:
            counts = torch.empty(n_rows, 2, dtype=torch.int32, device=dev)
        need = _lib.load().t2s_sos_scratch(n_rows, max_count, self.n_sections)
        scratch = torch.empty(need, dtype=torch.float64, device=dev)
        _lib.call("t2s_sos_filter", p(src), _KINDS[src.dtype], src.numel(), p(table4), n_rows, max_count, p(gains), p(self._tab(dev)),
                  self.n_sections, p(scratch), need, p(dst), _KINDS[dst.dtype], dst.numel(), max(1, int(max_out)), p(counts),
                  _lib.current_stream())
        return counts

    def filter_batch(self, audio, lengths=None, gain=None):
        """audio [N], [B, N] or [B, 1, N] float32 or float16 in HBM (strided rows are read where they are), lengths [B] (a device
        tensor is used where it is; None: whole rows) and gain (None, a float64 device tensor [B] or a number the samples are
        multiplied by first) -> (audio float32 of audio's shape, FilterReport(nonfinite, clipped int32 [B]) on the device): entry
        b's first lengths[b] samples filtered - forward(audio[b, :lengths[b]])'s bit for bit - and zeros behind them.  Samples at
        and behind lengths[b] are never read.  Nothing is read back."""
        what = "SosFilter.filter_batch"
        T2SError = _lib.T2SError
        if not torch.is_tensor(audio):
            raise T2SError("%s: audio must be a tensor, got a %s" % (what, type(audio).__name__))
        if torch.is_tensor(gain):
            if gain.dtype != torch.float64 or gain.dim() != 1 or gain.numel() != audio.numel() // max(1, audio.size(-1) if audio.dim() else 1):
                raise T2SError("%s: a gain tensor must be float64 [B], got %s %s" % (what, gain.dtype, tuple(gain.shape)))
            if gain.device != audio.device:
                raise T2SError("%s: gain is on %s, audio on %s" % (what, gain.device, audio.device))
        elif gain is not None and not _real(gain):
            raise T2SError("%s: gain must be None, a finite number or a float64 tensor [B] in HBM, got %r" % (what, gain))
        flat, B, N, ldx, lens_d = _float_rows(audio, lengths, what, "PcmPool.filter")
        if gain is None:
            gains = None
        elif torch.is_tensor(gain):
            gains = gain.detach().contiguous()
        else:
            gains = torch.full((B,), float(gain), dtype=torch.float64, device=flat.device)
        rows = torch.arange(B, dtype=torch.int64, device=flat.device)
        out = torch.empty(B, N, dtype=torch.float32, device=flat.device)
        table4 = torch.stack([rows * ldx, lens_d, rows * N, torch.full_like(rows, N)], 1).contiguous()
        counts = self._filter(flat, table4, B, N, gains, out.view(-1), N)
        return out.view(audio.shape), FilterReport(counts[:, 0], counts[:, 1])

    def forward(self, audio):
        """One clip [N] / [1, N], or whole rows [B, N] / [B, 1, N], float32 or float16 in HBM -> float32 of the same shape"""
        return self.filter_batch(audio, None)[0]

    __call__ = forward

    def stream(self):
        """A FilterStream of this filter: the row piece by piece, the pieces' outputs being forward(whole)'s bit for bit"""
        return FilterStream(self)


class FilterStream:
    """A SosFilter inside a stream: push(piece [B, n] float32 or float16 in HBM, last=False) -> [B, n] float32, for ANY piece
    lengths, 0 and 1 included; the concatenation of the outputs is filt.forward(whole) bit for bit, and after the last push report()
    is filter_batch's of the whole rows.  A causal filter holds nothing back: a push returns exactly n samples, and `last` only
    closes the stream.  The stream carries, in HBM and in two buffers used in turn, the cascade's state at the start of the row's
    current tile and the row's samples since then; a push filters carry | piece from the tile's start, which gives the whole row's
    bits because a lane's state in the scan depends on the lanes in front of it only.  Nothing is read back;
    every launch goes to the caller's current stream; B is fixed by the first push (or open())."""

    def __init__(self, filt):
        if not isinstance(filt, SosFilter):
            raise _lib.T2SError("FilterStream: filt must be an audio.SosFilter, got a %s" % type(filt).__name__)
        self.filter = filt
        self.B = None
        self.position = 0           # samples of the row seen so far (a host integer)
        self._ended = False
        self._order = _lib.StreamOrder()

    def open(self, B, device="cuda"):
        """Allocates the stream's carry for B rows and uploads the filter's table (the one blocking copy, where the filter has not
        uploaded it yet).  push() calls it with the first piece's B."""
        if self.B is not None:
            return self
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.T2SError("FilterStream: the stream's state lives in HBM (cuda); there is no CPU path")
        B = int(B)
        if not 1 <= B <= 65535:
            raise _lib.T2SError("FilterStream: %d rows, from 1 to 65535" % B)
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        lib = _lib.load()
        self._tile = lib.t2s_sos_tile()
        words = lib.t2s_sos_window_carry(self.filter.n_sections) // 8
        self._tab = self.filter._tab(dev)
        self._carry = [torch.zeros(B, words, dtype=torch.float64, device=dev) for _ in range(2)]
        self._counts = torch.zeros(B, 2, dtype=torch.int32, device=dev)
        self._ci = 0
        self.B, self.device = B, dev
        return self

    def report(self):
        """The running FilterReport (views of the stream's counts, int32 [B]) on the device"""
        if self.B is None:
            raise _lib.T2SError("FilterStream.report: nothing has been pushed yet")
        return FilterReport(self._counts[:, 0], self._counts[:, 1])

    def _tensors(self):
        return (self._carry, self._counts, self._tab)

    def _window(self, x, n, ldp):
        """The rows x (n samples each, ldp apart; opened, on the stream's device) -> out float32 [B, n]; no checks"""
        out = torch.empty(self.B, n, dtype=torch.float32, device=self.device)
        if n:
            lib, p, i = _lib.load(), _lib.ptr, self._ci
            need = lib.t2s_sos_scratch(self.B, self.position % self._tile + n, self.filter.n_sections)
            if need < 0:
                raise _lib.T2SError("FilterStream: a piece of %d samples, the most is 2^31 - 1 less a tile" % n)
            scratch = torch.empty(need, dtype=torch.float64, device=self.device)
            _lib.call("t2s_sos_window", p(self._carry[i]), p(self._carry[1 - i]), p(x), int(x.dtype == torch.float16), self.B, n, ldp,
                      self.position, None, p(self._tab), self.filter.n_sections, p(scratch), need, p(out), n, p(self._counts),
                      _lib.current_stream())
            self._ci = 1 - i
            self.position += n
        return out

    def push(self, piece, last=False):
        """piece [B, n] float32 or float16 in HBM (n may be 0; strided rows are read where they are) -> [B, n] float32.  Two
        launches (three where carry | piece fills a tile), on the caller's current stream; the host never waits."""
        T2SError = _lib.T2SError
        what = "FilterStream.push"
        if self._ended:
            raise T2SError("%s: a piece arrived behind the one flagged last" % what)
        if not torch.is_tensor(piece) or piece.dim() != 2:
            raise T2SError("%s: a piece must be a tensor [B, n], got %s" % (what, tuple(piece.shape) if torch.is_tensor(piece)
                                                                            else "a %s" % type(piece).__name__))
        if piece.dtype not in (torch.float32, torch.float16):
            raise T2SError("%s: expected float32 or float16, got %s" % (what, piece.dtype))
        _need_cuda(piece, what)
        B, n = piece.shape
        self.open(B, piece.device)
        if B != self.B or piece.device != self.device:
            raise T2SError("%s: the stream was opened for %d rows on %s, the piece has %d on %s"
                           % (what, self.B, self.device, B, piece.device))
        x = piece.detach()
        if n and (x.stride(1) != 1 or (B > 1 and x.stride(0) < n)):
            x = x.contiguous()
        ld = x.stride(0) if (B > 1 and n) else n
        cur = self._order.enter(self.device)
        if self._order.switched:
            _lib.record_stream(self._tensors(), cur)
        out = self._window(x, n, ld)
        self._ended = bool(last)
        return out


DELIVERY_ENCODINGS = ("f32", "pcm16", "ulaw", "alaw")


def _g711(audio, lengths, law):
    pcm = to_pcm16(audio, lengths)
    out = torch.empty(pcm.shape, dtype=torch.uint8, device=pcm.device)
    _lib.call("t2s_g711", _lib.ptr(pcm), pcm.numel(), law, _lib.ptr(out), _lib.current_stream())
    return out


def to_ulaw(audio, lengths=None):
    """Waveform in [-1, 1) -> G.711 mu-law bytes on the device: to_pcm16 (its arguments, its saturation) and then ITU-T G.711's
    integer algorithm on the int16 codes (t2s_g711, include/t2s_hip.h).  Returns a uint8 tensor of audio's shape."""
    return _g711(audio, lengths, 0)


def to_alaw(audio, lengths=None):
    """... -> G.711 A-law bytes (uint8 of audio's shape)"""
    return _g711(audio, lengths, 1)


class DeliveryStream:
    """The delivery chain inside a stream (csrc/delivery.hip): pieces of an utterance at `src_rate` in, pieces at `out_rate` out -
    resampled, multiplied by `gain`, limited by `limiter` and encoded - whose concatenation is, bit for bit,

        enc(limiter.limit_batch(Resampler(src_rate, out_rate).forward(whole), gain=gain)[0])

    for rows whose samples are finite and for ANY piece lengths, 0 and 1 included.  Both stages are local, so the stream keeps a
    short tail of each (ceil(n_taps / up) source samples; 2 limiter.reach delivery samples) in HBM from push to push; a piece is
    never resampled or limited alone, which would put a filter transient at every cut and lose the look-ahead across it.

    `out_rate` None or equal to src_rate skips the resampler.  `limiter` is an audio.Limiter built for the DELIVERY rate; `gain` a
    float or a float64 device tensor [B] (e.g. LoudnessReport.gain of a calibration utterance - the gated loudness of a programme
    is not known before it ends, so a stream cannot measure its own) and needs a limiter, as limit_batch(gain=) does.  `encoding`:
    "f32", "pcm16" (to_pcm16), "ulaw", "alaw" (to_ulaw / to_alaw).  At least one stage must be asked for.

    `pre_filter` and `post_filter` are audio.SosFilter cascades: the first runs at src_rate in front of the resampler (de-emphasis
    belongs here), the second at out_rate behind it and in front of the limiter (a filter changes peaks, so the limiter stays
    last; a telephone band in front of "ulaw" belongs here).  With them the concatenation is

        enc(limiter.limit_batch(post_filter.forward(Resampler(src_rate, out_rate).forward(pre_filter.forward(whole))), gain=gain)[0])

    bit for bit.  A causal filter holds nothing back: `latency` does not change.  filter_report() gives their counts.

    push(piece [B, n] float32 or float16 in HBM, last=False) -> [B, m] (float32 / int16 / uint8; m may be 0).  Until the piece
    flagged `last`, the stream holds back up to `latency` delivery samples: what the filters still need to see.  `delivered` counts
    the samples returned so far; both are host integers.  report() is the limiter's running LimiterReport on the device: after the
    last push it equals limiter.true_peak_batch's of the whole row.  A sample that is not finite cannot make the stream copy the
    row, as limit_batch does - it has already delivered - so the stream mutes around it (the gain goes to 0, what is stored is
    finite) and raises LIMIT_FLAG_NONFINITE.  Nothing is read back; every launch goes to the caller's current stream; B is fixed by
    the first push (or open()).  Not here: measured loudness, ragged batches, one launch for both stages."""

    def __init__(self, src_rate, out_rate=None, limiter=None, gain=None, encoding="f32", pre_filter=None, post_filter=None):
        T2SError = _lib.T2SError
        what = "DeliveryStream"
        for name, v in (("src_rate", src_rate),) + ((("out_rate", out_rate),) if out_rate is not None else ()):
            try:
                whole = not isinstance(v, bool) and int(v) == v and v >= 1
            except (TypeError, ValueError, OverflowError):
                whole = False
            if not whole:
                raise T2SError("%s: %s must be a positive integer, got %r" % (what, name, v))
        self.src_rate = int(src_rate)
        self.out_rate = self.src_rate if out_rate is None else int(out_rate)
        if encoding not in DELIVERY_ENCODINGS:
            raise T2SError("%s: encoding must be one of %s, got %r" % (what, ", ".join(DELIVERY_ENCODINGS), encoding))
        if limiter is not None and not isinstance(limiter, Limiter):
            raise T2SError("%s: limiter must be an audio.Limiter or None, got a %s" % (what, type(limiter).__name__))
        if limiter is not None and limiter.sampling_rate != self.out_rate:
            raise T2SError("%s: the limiter was built for %d Hz, the delivery rate is %d Hz (limit last, at the rate delivered)"
                           % (what, limiter.sampling_rate, self.out_rate))
        if gain is not None:
            if limiter is None:
                raise T2SError("%s: gain needs a limiter (the gain is applied inside it, as limit_batch(gain=) does)" % what)
            if torch.is_tensor(gain):
                if gain.dtype != torch.float64 or gain.dim() != 1 or gain.numel() == 0:
                    raise T2SError("%s: a gain tensor must be float64 [B], got %s %s" % (what, gain.dtype, tuple(gain.shape)))
            elif not _real(gain):
                raise T2SError("%s: gain must be a finite number or a float64 tensor [B], got %r" % (what, gain))
        self.up = self.down = 1
        self._h_host = None
        if self.out_rate != self.src_rate:
            self.up, self.down, self._h_host = resample_filter(self.src_rate, self.out_rate)
            if max(self.up, self.down) > RESAMPLE_MAX_FACTOR:
                raise T2SError("%s: %d -> %d Hz is the ratio %d / %d; max(up, down) may be at most %d"
                               % (what, self.src_rate, self.out_rate, self.up, self.down, RESAMPLE_MAX_FACTOR))
        for name, filt, rate in (("pre_filter", pre_filter, self.src_rate), ("post_filter", post_filter, self.out_rate)):
            if filt is None:
                continue
            if not isinstance(filt, SosFilter):
                raise T2SError("%s: %s must be an audio.SosFilter or None, got a %s" % (what, name, type(filt).__name__))
            if filt.sampling_rate is not None and filt.sampling_rate != rate:
                raise T2SError("%s: %s was designed for %g Hz, it runs at %d Hz (pre_filter at src_rate, post_filter at out_rate)"
                               % (what, name, filt.sampling_rate, rate))
        if self._h_host is None and limiter is None and encoding == "f32" and pre_filter is None and post_filter is None:
            raise T2SError("%s: nothing to do - ask for another rate, a limiter or an encoding" % what)
        self.limiter, self.gain, self.encoding = limiter, gain, encoding
        self.pre_filter, self.post_filter = pre_filter, post_filter
        self._pre = self._post = None       # their FilterStreams, made by open()
        self.n_taps = 0 if self._h_host is None else int(self._h_host.size)
        # the carries: host arithmetic (the library's t2s_*_window_carry restate it and the tests compare)
        self.resample_carry = 0 if self._h_host is None else -(-self.n_taps // self.up)
        self.limit_carry = 0 if limiter is None else 2 * limiter.reach
        # delivery samples a push may hold back: the outputs whose last tap the source has not reached, and the limiter's reach
        self.latency = (0 if self._h_host is None else -(-(self.n_taps // 2) // self.down)) + (0 if limiter is None else limiter.reach)
        self.delivered = 0
        self.B = None
        self._ended = False
        self._K = self._M = self._N = self._O = 0      # source samples seen, resampled; delivery samples seen, limited
        self._order = _lib.StreamOrder()

    def open(self, B, device="cuda"):
        """Allocates the stream's state for B rows and uploads the tables (the one blocking copy, where the limiter has not
        uploaded its own yet).  push() calls it with the first piece's B; call it first where not even that push may block."""
        if self.B is not None:
            return self
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.T2SError("DeliveryStream: the stream's state lives in HBM (cuda); there is no CPU path")
        B = int(B)
        if not 1 <= B <= 65535:
            raise _lib.T2SError("DeliveryStream: %d rows, from 1 to 65535" % B)
        if dev.index is None:                                   # ("cuda": the current device, named as a piece's .device names it)
            dev = torch.device("cuda", torch.cuda.current_device())
        self._gains = None
        if self.gain is not None:
            if torch.is_tensor(self.gain):
                if self.gain.numel() != B or self.gain.device.type != "cuda":
                    raise _lib.T2SError("DeliveryStream: gain holds %d values on %s, the stream has %d rows in HBM"
                                        % (self.gain.numel(), self.gain.device, B))
                self._gains = self.gain.detach().contiguous()
            else:
                self._gains = torch.full((B,), float(self.gain), dtype=torch.float64, device=dev)
        self._h = None if self._h_host is None else _to_device(torch.from_numpy(self._h_host), dev)
        # (ping-pong: a window reads one carry and writes the other; zeros, though samples below index 0 are never read)
        self._rc = [torch.zeros(B, self.resample_carry, dtype=torch.float32, device=dev) for _ in range(2)] if self._h is not None else None
        self._lc = self._state = None
        if self.limiter is not None:
            self.limiter._hw(dev)
            self._lc = [torch.zeros(B, self.limit_carry, dtype=torch.float32, device=dev) for _ in range(2)]
            self._state = torch.zeros(B, 5, dtype=torch.int64, device=dev)
            self._state[:, 2].fill_(0x3FF0000000000000)         # the bits of 1.0: the smallest gain so far
        self._ri = self._li = 0
        if self.pre_filter is not None:
            self._pre = self.pre_filter.stream().open(B, dev)
        if self.post_filter is not None:
            self._post = self.post_filter.stream().open(B, dev)
        self.B, self.device = B, dev
        return self

    def report(self):
        """The limiter's running state as a LimiterReport of views into it (float64 [B] x 3, int32 [B] x 2), on the device"""
        if self.limiter is None:
            raise _lib.T2SError("DeliveryStream.report: the stream has no limiter")
        if self.B is None:
            raise _lib.T2SError("DeliveryStream.report: nothing has been pushed yet")
        return Limiter._report(self._state[:, :4].view(torch.float64), self._state[:, 4:].view(torch.int32))

    def filter_report(self):
        """(pre_filter's running FilterReport or None, post_filter's or None), views on the device"""
        if self.B is None:
            raise _lib.T2SError("DeliveryStream.filter_report: nothing has been pushed yet")
        return tuple(None if fs is None else fs.report() for fs in (self._pre, self._post))

    def _resample(self, x, n, ldp, final):
        lib, p = _lib.load(), _lib.ptr
        M1 = lib.t2s_resample_window_end(self._K + n, self._M, self.n_taps, self.up, self.down, int(final))
        m = M1 - self._M
        out = torch.empty(self.B, m, dtype=torch.float32, device=self.device)
        if n or m:
            i = self._ri
            _lib.call("t2s_resample_window", p(self._rc[i]), p(self._rc[1 - i]), p(x) if n else None, int(x.dtype == torch.float16),
                      self.B, n, ldp, self._K, self._M, int(final), p(self._h), self.n_taps, self.up, self.down,
                      p(out) if m else None, m, m, _lib.current_stream())
            self._ri = 1 - i
        self._K += n
        self._M = M1
        return out, m, m

    def _limit(self, x, n, ldp, final):
        lib, p, lim = _lib.load(), _lib.ptr, self.limiter
        O1 = lib.t2s_limit_window_end(self._N + n, self._O, lim.lookahead, lim.half_width, int(final))
        m = O1 - self._O
        out = torch.empty(self.B, m, dtype=torch.float32, device=self.device)
        if n or m:
            i = self._li
            _lib.call("t2s_limit_window", p(self._lc[i]), p(self._lc[1 - i]), p(x) if n else None, int(x.dtype == torch.float16),
                      self.B, n, ldp, self._N, self._O, int(final), p(self._gains), *lim._params(self.device),
                      p(out) if m else None, m, m, p(self._state), _lib.current_stream())
            self._li = 1 - i
        self._N += n
        self._O = O1
        return out, m, m

    def push(self, piece, last=False):
        """piece [B, n] float32 or float16 in HBM (n may be 0; strided rows are read where they are) -> what can be delivered now,
        [B, m] in the stream's encoding, m >= 0.  `last` ends the row: what was held back comes out, and no further piece is
        taken.  One launch a stage and one or two for the encoding, on the caller's current stream; the host never waits."""
        T2SError = _lib.T2SError
        what = "DeliveryStream.push"
        if self._ended:
            raise T2SError("%s: a piece arrived behind the one flagged last" % what)
        if not torch.is_tensor(piece) or piece.dim() != 2:
            raise T2SError("%s: a piece must be a tensor [B, n], got %s" % (what, tuple(piece.shape) if torch.is_tensor(piece)
                                                                            else "a %s" % type(piece).__name__))
        if piece.dtype not in (torch.float32, torch.float16):
            raise T2SError("%s: expected float32 or float16, got %s" % (what, piece.dtype))
        _need_cuda(piece, what)
        B, n = piece.shape
        self.open(B, piece.device)
        if B != self.B or piece.device != self.device:
            raise T2SError("%s: the stream was opened for %d rows on %s, the piece has %d on %s"
                           % (what, self.B, self.device, B, piece.device))
        x = piece.detach()
        if n and (x.stride(1) != 1 or (B > 1 and x.stride(0) < n)):
            x = x.contiguous()
        ld = x.stride(0) if (B > 1 and n) else n
        cur = self._order.enter(self.device)
        if self._order.switched:
            _lib.record_stream((self._rc, self._lc, self._state, self._h, self._gains), cur)
            for fs in (self._pre, self._post):
                if fs is not None:
                    _lib.record_stream(fs._tensors(), cur)
        final = bool(last)
        if self._pre is not None:
            x, ld = self._pre._window(x, n, ld), n
        if self._h is not None:
            x, n, ld = self._resample(x, n, ld, final)
        if self._post is not None:
            x, ld = self._post._window(x, n, ld), n
        if self.limiter is not None:
            x, n, ld = self._limit(x, n, ld, final)
        self._ended = final
        self.delivered += n
        if self.encoding == "f32":
            return x
        if n == 0:
            return torch.empty(B, 0, dtype=torch.int16 if self.encoding == "pcm16" else torch.uint8, device=self.device)
        if self.encoding == "pcm16":
            return to_pcm16(x)
        return to_ulaw(x) if self.encoding == "ulaw" else to_alaw(x)


JOIN_MAX_FADE = 65536          # the library's limit on the fade (include/t2s_hip.h)
JOIN_MAX_SAMPLES = 2 ** 31 - 1  # ... and on the joined row


def _join_count(v, what, name):
    """a host count of samples (or a row number) as an int >= 0; anything else raises ValueError"""
    try:
        n = None if isinstance(v, bool) else operator.index(v)
    except TypeError:
        n = None
    if n is None:
        raise ValueError("%s: %s must be an integer, got a %s" % (what, name, type(v).__name__))
    if n < 0:
        raise ValueError("%s: %s must not be negative, got %d" % (what, name, n))
    return n


def _join_rows(audio, lengths, k, what):
    """One source batch of join_batches, checked -> (rows [B, N], B, N, lengths as given: a device tensor or a host one)"""
    T2SError = _lib.T2SError
    who = "%s: batch %d" % (what, k)
    _need_cuda(audio, who)
    if audio.dim() not in (2, 3) or (audio.dim() == 3 and audio.size(1) != 1) or audio.numel() == 0:
        raise T2SError("%s: audio must be [B, N] or [B, 1, N] and hold samples, got %s" % (who, tuple(audio.shape)))
    x = audio.detach()
    if x.dtype not in (torch.float32, torch.float16):
        raise T2SError("%s: expected float32 or float16, got %s (there is no silent cast)" % (who, x.dtype))
    N = x.size(-1)
    x = x.reshape(-1, N)
    B = x.size(0)
    try:
        lens = torch.as_tensor(lengths)
    except (TypeError, ValueError, RuntimeError) as e:
        raise T2SError("%s: lengths must be a tensor or a sequence of integers (%s)" % (who, e))
    if lens.is_floating_point() or lens.is_complex() or lens.dtype == torch.bool:
        raise T2SError("%s: lengths must be integers, got %s" % (who, lens.dtype))
    if lens.dim() != 1 or lens.numel() != B:
        raise T2SError("%s: lengths has shape %s, the batch holds %d entries" % (who, tuple(lens.shape), B))
    if lens.device.type != "cpu" and lens.device != x.device:
        raise T2SError("%s: lengths live on %s, the audio on %s" % (who, lens.device, x.device))
    return x, B, N, lens.detach()


def join_batches(batches, order=None, pause=0, pauses=None, fade=0, fade_ends=False):
    """The rows of padded batches as ONE utterance in HBM: segment after segment, `pause` samples of silence between them, a linear
    ramp of `fade` samples at the joints (csrc/join.hip; include/t2s_hip.h states the arithmetic).  `batches`: a list of
    (audio [B, N] or [B, 1, N] float32 or float16 in HBM, lengths [B]) - WaveGlow.infer_batch's, Denoiser.denoise_batch's or
    Trimmer.trim_batch's two results as returned.  A device tensor of lengths is used where it is (clamped to [0, N] on the device);
    a host tensor or a sequence is copied over.  Rows are numbered through the batches in the order given, n in all.

    order    a host sequence, a permutation of the n rows: position -> row (None: the rows as numbered)
    pause    samples of silence behind every segment but the last; `pauses`: n - 1 host ints by position, instead
    fade     samples of ramp r(k) = (2k + 1) / (2 fade) at the start of every segment but the first and at the end of every segment
             but the last; `fade_ends`: at the utterance's own two ends as well.  A segment shorter than 2 fade gets both factors.

    Returns (audio float32 [1, cap], length int32 [1] on the device, offsets int64 [n + 1] on the device): segment p is
    audio[0, offsets[p] : offsets[p] + its length], offsets[n] = length the joined samples, and everything else up to
    cap = sum B N + sum of the pauses - known on the host - is +0.  With fade = 0 a segment's samples are copied bit for bit (f16
    widened exactly); whatever the fade they depend on the segment, the fade and whether it is first or last - not on its batch or
    row.  Nothing is read back: one small host-to-device copy (the order, the pauses), one scan launch and one gather launch per
    batch, all on the current stream."""
    what = "join_batches"
    T2SError = _lib.T2SError
    try:
        batches = [tuple(b) for b in batches]
    except TypeError:
        raise T2SError("%s: batches must be a list of (audio, lengths) pairs" % what) from None
    if not batches or any(len(b) != 2 for b in batches):
        raise T2SError("%s: batches must be a non-empty list of (audio, lengths) pairs" % what)
    fade = _join_count(fade, what, "fade")
    if fade > JOIN_MAX_FADE:
        raise ValueError("%s: fade may be at most %d samples, got %d" % (what, JOIN_MAX_FADE, fade))
    rows = [_join_rows(a, l, k, what) for k, (a, l) in enumerate(batches)]
    dev = rows[0][0].device
    for k, r in enumerate(rows):
        if r[0].device != dev:
            raise T2SError("%s: batch %d is on %s, batch 0 on %s" % (what, k, r[0].device, dev))
    n = sum(r[1] for r in rows)
    if n > 65535:
        raise T2SError("%s: %d rows, the most is 65535" % (what, n))
    if pauses is not None:
        try:
            gaps = [_join_count(g, what, "a pause") for g in pauses]
        except TypeError:
            raise ValueError("%s: pauses must be a sequence of integers" % what) from None
        if len(gaps) != n - 1:
            raise ValueError("%s: pauses holds %d values, %d segments need %d" % (what, len(gaps), n, n - 1))
    else:
        gaps = [_join_count(pause, what, "pause")] * (n - 1)
    if order is None:
        order = list(range(n))
    else:
        try:
            order = [_join_count(r, what, "an entry of order") for r in order]
        except TypeError:
            raise ValueError("%s: order must be a sequence of integers" % what) from None
        if sorted(order) != list(range(n)):
            raise ValueError("%s: order must be a permutation of the %d rows, got %s" % (what, n, order))
    cap = sum(r[1] * r[2] for r in rows) + sum(gaps)
    if cap > JOIN_MAX_SAMPLES:
        raise T2SError("%s: the joined row would hold %d samples, the most is %d" % (what, cap, JOIN_MAX_SAMPLES))
    pos = [0] * n
    for p, r in enumerate(order):
        pos[r] = p
    caps = [r[2] for r in rows for _ in range(r[1])]
    # one table, one copy: order | pos | caps | pauses, then every host tensor of lengths
    host = [torch.tensor(order + pos + caps + gaps, dtype=torch.int32)]
    host += [r[3].to(torch.int64).clamp(0, r[2]).to(torch.int32) for r in rows if not r[3].is_cuda]
    table = _to_device(torch.cat(host), dev)
    order_d, pos_d, caps_d, gaps_d = table[:n], table[n:2 * n], table[2 * n:3 * n], table[3 * n:4 * n - 1]
    at = 4 * n - 1
    lens_d = []
    for r in rows:
        if r[3].is_cuda:
            lens_d.append(r[3].clamp(0, r[2]).to(torch.int32))
        else:
            lens_d.append(table[at:at + r[1]])
            at += r[1]
    all_lens = lens_d[0] if len(rows) == 1 else torch.cat(lens_d)
    out = torch.empty(1, cap, dtype=torch.float32, device=dev)
    length = torch.empty(1, dtype=torch.int32, device=dev)
    offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    p, st = _lib.ptr, _lib.current_stream()
    _lib.call("t2s_join_offsets", p(all_lens), p(caps_d), p(order_d), p(gaps_d) if n > 1 else None, 0, n, p(out), cap, p(offsets),
              p(length), st)
    r0 = 0
    for (x, B, N, _), lens in zip(rows, lens_d):
        if x.stride(1) != 1 or (B > 1 and x.stride(0) < N):
            x = x.contiguous()
        _lib.call("t2s_join_gather", p(x), _KINDS[x.dtype], B, N, x.stride(0) if B > 1 else N, p(lens), p(pos_d[r0:r0 + B]), p(offsets),
                  n, fade, int(bool(fade_ends)), p(out), cap, st)
        r0 += B
    return out, length, offsets


def join_batch(audio, lengths, order=None, pause=0, pauses=None, fade=0, fade_ends=False):
    """join_batches for one batch: the rows of (audio, lengths) as one utterance."""
    return join_batches([(audio, lengths)], order, pause, pauses, fade, fade_ends)


def dynamic_range_compression(x, C=1, clip_val=1e-5):
    return torch.log(torch.clamp(x, min=clip_val) * C)


def dynamic_range_decompression(x, C=1):
    return torch.exp(x) / C


def mel_filterbank(sr, n_fft, n_mels=80, fmin=0.0, fmax=None):
    """Triangular mel filters [n_mels, 1 + n_fft/2], Slaney scale and area normalisation (librosa.filters.mel defaults)."""
    fmax = float(sr) / 2 if fmax is None else float(fmax)
    f_sp, brk = 200.0 / 3.0, 1000.0
    step = np.log(6.4) / 27.0

    def to_mel(hz):
        hz = np.asarray(hz, dtype=np.float64)
        return np.where(hz < brk, hz / f_sp, brk / f_sp + np.log(np.maximum(hz, 1e-10) / brk) / step)

    def to_hz(mel):
        mel = np.asarray(mel, dtype=np.float64)
        return np.where(mel < brk / f_sp, mel * f_sp, brk * np.exp(step * (mel - brk / f_sp)))

    edges = to_hz(np.linspace(to_mel(fmin), to_mel(fmax), n_mels + 2))          # n_mels + 2 band edges in Hz
    bins = np.linspace(0.0, float(sr) / 2, 1 + n_fft // 2)
    rise = (bins[None, :] - edges[:-2, None]) / (edges[1:-1] - edges[:-2])[:, None]
    fall = (edges[2:, None] - bins[None, :]) / (edges[2:] - edges[1:-1])[:, None]
    tri = np.clip(np.minimum(rise, fall), 0.0, None)
    tri *= (2.0 / (edges[2:] - edges[:-2]))[:, None]
    return tri.astype(np.float32)


def griffin_lim(magnitudes, stft_fn, n_iters=30, angles=None):
    """Phase reconstruction by alternating projections (reference utils/audio_processing.py:50-72): every transform and
    inverse runs on the device.  `angles` (radians, same shape as `magnitudes`) replaces the reference's random initial phase
    when given, which makes the result reproducible."""
    _need_cuda(magnitudes, "griffin_lim")
    if angles is None:
        angles = torch.rand(magnitudes.shape, device=magnitudes.device, dtype=torch.float32) * (2 * np.pi) - np.pi
    signal = stft_fn.inverse(magnitudes, angles).squeeze(1)
    for _ in range(n_iters):
        _, angles = stft_fn.transform(signal)
        signal = stft_fn.inverse(magnitudes, angles).squeeze(1)
    return signal


class STFT(torch.nn.Module):
    """Short-time Fourier transform as a strided contraction with a windowed Fourier basis (reference utils/stft.py:36)."""

    def __init__(self, filter_length=800, hop_length=200, win_length=800, window="hann"):
        super().__init__()
        if filter_length % 16 or hop_length % 4:
            raise ValueError("filter_length must be a multiple of 16 and hop_length a multiple of 4")
        self.filter_length, self.hop_length, self.win_length, self.window = filter_length, hop_length, win_length, window
        self.forward_transform = None
        scale = filter_length / hop_length
        fourier = np.fft.fft(np.eye(filter_length))
        cutoff = filter_length // 2 + 1
        fourier = np.vstack([fourier[:cutoff].real, fourier[:cutoff].imag])
        fwd = torch.FloatTensor(fourier[:, None, :])
        inv = torch.FloatTensor(np.linalg.pinv(scale * fourier).T[:, None, :])
        win_sq = None
        if window is not None:
            if filter_length < win_length:
                raise ValueError("filter_length < win_length")
            w = get_window(window, win_length, fftbins=True)
            lpad = (filter_length - win_length) // 2
            w = np.pad(w, (lpad, filter_length - win_length - lpad))        # librosa.util.pad_center
            wt = torch.from_numpy(w).float()
            fwd = fwd * wt
            inv = inv * wt
            win_sq = torch.from_numpy((w ** 2).astype(np.float32))
        self.register_buffer("forward_basis", fwd.float())
        self.register_buffer("inverse_basis", inv.float())
        # device-side operands: inverse basis transposed [n_fft][ld_rc] (zero padded), squared window
        self._ld_rc = _ru(2 * cutoff, 16)
        inv_t = torch.zeros(filter_length, self._ld_rc)
        inv_t[:, :2 * cutoff] = inv[:, 0, :].t()
        self.register_buffer("_inv_basis_t", inv_t, persistent=False)
        self.register_buffer("_win_sq", win_sq if win_sq is not None else torch.zeros(0), persistent=False)

    # -- helpers ------------------------------------------------------------------------------------------------------
    # Without lengths a call is the whole batch at its full extent.  With them (a padded batch), entry b gets what it gets alone
    # (bit for bit: the same kernels' arithmetic on its own extent, the contractions launched at its own frame count) whatever the
    # padding holds, and zeros behind its end.
    def _transform(self, input_data, lens=None, want_mag=True, want_phase=True, ld_mt=0):
        """`lens`: None, or validated host int64 [B] (samples).  Returns (mag, phase, magT, F, frame counts: host int64 [B], None
        without `lens`)."""
        _need_cuda(input_data, "STFT.transform")
        _need_cuda(self.forward_basis, "STFT (call .cuda() on the module)")
        x = input_data.detach().to(torch.float32).contiguous()
        B, T = x.shape
        n_fft, hop = self.filter_length, self.hop_length
        c, F = n_fft // 2 + 1, T // hop + 1
        dev = x.device
        ldp = _ru(T + n_fft, 4)
        xp = torch.empty(B, ldp, device=dev)
        ft = torch.empty(B, F, 2 * c, device=dev)
        mag = torch.empty(B, c, F, device=dev) if want_mag else None
        ph = torch.empty(B, c, F, device=dev) if want_phase else None
        magT = torch.empty(B * F, ld_mt, device=dev) if ld_mt else None
        p = _lib.ptr
        rest = (p(self.forward_basis), n_fft, hop, p(xp), ldp, p(ft), p(mag), p(ph), p(magT), ld_mt, _lib.current_stream())
        if lens is None:
            _lib.call("t2s_stft_transform", p(x), B, T, *rest)
            self._keep = (x, xp, ft)
            return mag, ph, magT, F, None
        lens_d, lens_h = _both(lens, dev)
        _lib.call("t2s_stft_transform_ragged", p(x), B, T, p(lens_d), p(lens_h), *rest)
        self._keep = (x, xp, ft, lens_d)
        return mag, ph, magT, F, lens // hop + 1

    def _inverse(self, magnitude, phase, fl=None, _bias=None, _strength=0.0):
        """`fl`: None, or validated host int64 [B] (frames, in [2, F]).  Returns audio [B, 1, hop (F - 1)]."""
        mag = magnitude.detach().to(torch.float32).contiguous()
        ph = phase.detach().to(torch.float32).contiguous()
        B, c, F = mag.shape
        n_fft, hop = self.filter_length, self.hop_length
        dev = mag.device
        rc = torch.empty(B * F, self._ld_rc, device=dev)
        frames = torch.empty(B, F, n_fft, device=dev)
        out = torch.empty(B, 1, hop * (F - 1), device=dev)
        p = _lib.ptr
        rest = (n_fft, hop, p(self._inv_basis_t), self._ld_rc, p(_bias), float(_strength),
                p(self._win_sq) if self.window is not None else None, float(np.finfo(np.float32).tiny), p(rc), p(frames), p(out),
                _lib.current_stream())
        if fl is None:
            _lib.call("t2s_stft_inverse", p(mag), p(ph), B, F, *rest)
            self._keep_inv = (mag, ph, rc, frames, _bias)
            return out
        fl_d, fl_h = _both(fl, dev)
        _lib.call("t2s_stft_inverse_ragged", p(mag), p(ph), B, F, p(fl_d), p(fl_h), *rest)
        self._keep_inv = (mag, ph, rc, frames, _bias, fl_d)
        return out

    # -- reference surface --------------------------------------------------------------------------------------------
    def transform(self, input_data):
        """audio [B, T] -> (magnitude, phase), each [B, filter_length/2 + 1, 1 + T // hop_length]"""
        self.num_samples = input_data.size(1)
        mag, ph, _, _, _ = self._transform(input_data)
        return mag, ph

    def inverse(self, magnitude, phase, _bias=None, _strength=0.0):
        """(magnitude, phase) -> audio [B, 1, hop_length * (frames - 1)]"""
        _need_cuda(magnitude, "STFT.inverse")
        return self._inverse(magnitude, phase, None, _bias, _strength)

    def forward(self, input_data):
        self.magnitude, self.phase = self.transform(input_data)
        return self.inverse(self.magnitude, self.phase)

    # -- padded batches of different lengths ----------------------------------------------------------------------------
    def _batch_audio(self, audio, lengths, what):
        """[B, T] or [B, 1, T] in HBM and its lengths -> ([B, T], validated host int64 lengths in (filter_length / 2, T])"""
        _need_cuda(audio, what)
        if audio.dim() == 3 and audio.size(1) == 1:
            audio = audio[:, 0]
        if audio.dim() != 2:
            raise _lib.T2SError("%s: audio must be [B, T] or [B, 1, T], got %s" % (what, tuple(audio.shape)))
        B, T = audio.shape
        # (an entry of at most filter_length / 2 samples cannot be reflect-padded: the solo call refuses it too)
        return audio, _host_lengths(lengths, B, self.filter_length // 2 + 1, T, what, "samples")

    def transform_batch(self, audio, lengths):
        """audio [B, T] padded, lengths [B] -> (magnitude, phase, frame_lengths): entry b's first 1 + lengths[b] // hop_length
        frames are transform(audio[b:b+1, :lengths[b]])'s, the rest zeros; frame_lengths int64 [B] on the device."""
        audio, lens = self._batch_audio(audio, lengths, "STFT.transform_batch")
        mag, ph, _, _, fl = self._transform(audio, lens)
        return mag, ph, fl.to(audio.device)

    def inverse_batch(self, magnitude, phase, frame_lengths):
        """(magnitude, phase) [B, filter_length/2 + 1, F] padded, frame_lengths [B] in [2, F] -> (audio [B, 1, hop (F - 1)],
        audio_lengths): entry b's first hop (frame_lengths[b] - 1) samples are inverse() of its own frames, the rest zeros;
        frames behind an entry's end are not read.  audio_lengths int64 [B] on the device."""
        what = "STFT.inverse_batch"
        _need_cuda(magnitude, what)
        _need_cuda(phase, what)
        if magnitude.dim() != 3 or magnitude.shape != phase.shape or magnitude.size(1) != self.filter_length // 2 + 1:
            raise _lib.T2SError("%s: magnitude and phase must both be [B, %d, F], got %s and %s"
                                % (what, self.filter_length // 2 + 1, tuple(magnitude.shape), tuple(phase.shape)))
        B, _, F = magnitude.shape
        fl = _host_lengths(frame_lengths, B, 2, F, what, "frames")
        out = self._inverse(magnitude, phase, fl)
        return out, ((fl - 1) * self.hop_length).to(out.device)


class TacotronSTFT(torch.nn.Module):
    """log-mel spectrogram of the reference (utils/layers.py:42-79)."""

    def __init__(self, filter_length=1024, hop_length=256, win_length=1024, n_mel_channels=80, sampling_rate=44800, mel_fmin=0.0,
                 mel_fmax=8000.0):
        super().__init__()
        self.n_mel_channels, self.sampling_rate = n_mel_channels, sampling_rate
        self.stft_fn = STFT(filter_length, hop_length, win_length)
        mel_basis = torch.from_numpy(mel_filterbank(sampling_rate, filter_length, n_mel_channels, mel_fmin, mel_fmax)).float()
        self.register_buffer("mel_basis", mel_basis)
        self._ld_mt = _ru(filter_length // 2 + 1, 16)
        mp = torch.zeros(n_mel_channels, self._ld_mt)
        mp[:, :mel_basis.size(1)] = mel_basis
        self.register_buffer("_mel_basis_p", mp, persistent=False)

    def spectral_normalize(self, magnitudes):
        return dynamic_range_compression(magnitudes)

    def spectral_de_normalize(self, magnitudes):
        return dynamic_range_decompression(magnitudes)

    def mel_spectrogram(self, y):
        """y [B, T] in [-1, 1] (in HBM) -> log-mel [B, n_mel_channels, 1 + T // hop]"""
        _need_cuda(y, "TacotronSTFT.mel_spectrogram")
        # the reference asserts the range on the host (utils/layers.py:72-73); one fused device reduction here
        lo, hi = torch.aminmax(y.detach())
        if float(lo) < -1 or float(hi) > 1:
            raise AssertionError("audio outside [-1, 1]")
        return self._mel(y)[0]

    def _mel(self, y, lens=None):
        """y [B, T] and None or validated host int64 lengths -> (log-mel [B, n_mel_channels, F], frame counts as STFT._transform's)"""
        _, _, magT, F, fl = self.stft_fn._transform(y, lens, want_mag=False, want_phase=False, ld_mt=self._ld_mt)
        B = y.size(0)
        mel = torch.empty(B, self.n_mel_channels, F, device=y.device)
        p = _lib.ptr
        rest = (p(self._mel_basis_p), self.n_mel_channels, 1e-5, p(mel), _lib.current_stream())
        if fl is None:
            _lib.call("t2s_mel_from_mag", p(magT), self._ld_mt, B, F, *rest)
            self._keep = magT
        else:
            fl_d, fl_h = _both(fl, y.device)
            _lib.call("t2s_mel_from_mag_ragged", p(magT), self._ld_mt, B, F, p(fl_d), p(fl_h), *rest)
            self._keep = (magT, fl_d)
        return mel, fl

    def mel_spectrogram_batch(self, y, lengths):
        """y [B, T] padded (in HBM), lengths [B] -> (mel [B, n_mel_channels, 1 + T // hop], mel_lengths): entry b's first
        1 + lengths[b] // hop columns are mel_spectrogram(y[b:b+1, :lengths[b]])'s, the columns behind are zeros (what the
        reference's collate pads with, not log(clip)).  The [-1, 1] assertion judges the valid samples; the padding may hold
        anything.  mel_lengths int64 [B] on the device."""
        what = "TacotronSTFT.mel_spectrogram_batch"
        y, lens = self.stft_fn._batch_audio(y, lengths, what)
        B, T = y.shape
        lens_d = lens.to(y.device)
        valid = torch.arange(T, device=y.device)[None, :] < lens_d[:, None]
        lo, hi = torch.aminmax(torch.where(valid, y.detach(), torch.zeros((), dtype=y.dtype, device=y.device)))
        if float(lo) < -1 or float(hi) > 1:
            raise AssertionError("audio outside [-1, 1]")
        mel, fl = self._mel(y, lens)
        return mel, fl.to(y.device)


class Denoiser(torch.nn.Module):
    """Removes the vocoder's bias spectrum from its output (waveglow/denoiser.py:7-40)."""

    def __init__(self, waveglow, filter_length=1024, n_overlap=4, win_length=1024, mode="zeros"):
        super().__init__()
        w = waveglow.upsample.weight
        self.stft = STFT(filter_length=filter_length, hop_length=int(filter_length / n_overlap), win_length=win_length).to(w.device)
        if mode == "zeros":
            mel_input = torch.zeros((1, 80, 88), dtype=w.dtype, device=w.device)
        elif mode == "normal":
            mel_input = torch.randn((1, 80, 88), dtype=w.dtype, device=w.device)
        else:
            raise Exception("Mode {} if not supported".format(mode))
        with torch.no_grad():
            bias_audio = waveglow.infer(mel_input, sigma=0.0).float()
            bias_spec, _ = self.stft.transform(bias_audio)
        self.register_buffer("bias_spec", bias_spec[:, :, 0][:, :, None].contiguous())

    def forward(self, audio, strength=0.1):
        _need_cuda(audio, "Denoiser.forward")
        mag, ph = self.stft.transform(audio.float())
        # spectral subtraction + clamp are fused into the recombination kernel of the inverse transform
        return self.stft.inverse(mag, ph, _bias=self.bias_spec.reshape(-1).contiguous(), _strength=strength)

    def denoise_batch(self, audio, lengths, strength=0.1):
        """forward() on a padded batch: audio [B, T] (or [B, 1, T]) float32 or float16 and lengths [B], e.g. WaveGlow.infer_batch's
        two results as returned.  Returns (audio [B, 1, hop (T // hop)] float32, audio_lengths int64 [B] on the device): entry b's
        first hop (lengths[b] // hop) samples are forward(audio[b:b+1, :lengths[b]], strength)'s bit for bit - its reflect padding
        mirrors about its own end and its overlap-add counts its own frames - and the rest of its row is zeros.  An entry of at
        most filter_length / 2 samples is refused, as forward() refuses it alone."""
        what = "Denoiser.denoise_batch"
        audio, lens = self.stft._batch_audio(audio, lengths, what)
        mag, ph, _, _, fl = self.stft._transform(audio.float(), lens)
        out = self.stft._inverse(mag, ph, fl, _bias=self.bias_spec.reshape(-1).contiguous(), _strength=strength)
        return out, _to_device((fl - 1) * self.stft.hop_length, out.device)
