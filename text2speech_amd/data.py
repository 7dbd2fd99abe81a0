"""Training batches assembled on the MI355X from int16 PCM: a corpus of clips lives in HBM, and one call turns
a list of clip indices into the tensors `WaveGlow.forward` / `Tacotron.forward` take.

  PcmPool(clips, sampling_rate)                 the clips back to back in one int16 device tensor; .from_wav_files(paths, rate);
                                                .resample(new_rate) / from_wav_files(..., resample=True): rate conversion in HBM;
                                                .rescale_trim(rescaling_max, top_db): the reference's peak rescaling and silence trim
                                                .loudness() / .normalize_loudness(target_lufs): BS.1770 gated loudness per clip
                                                .true_peak(limiter) / .limit(limiter, loudness): true peak and look-ahead limiter
  Mel2SampBatch(pool, segment_length, ...)      waveglow/mel2samp.py:60-105 (Mel2Samp.__getitem__ + the default collate): (mel, audio)
  TextMelBatch(pool, sequences, ...)            utils/data_utils.py:46-150 (TextMelLoader + TextMelCollate) and Tacotron.parse_batch

Cropping, zero padding, the division by max_wav_value (t2s_pcm16_gather), the mels (TacotronSTFT) and the gate targets
(t2s_gate_targets) run in libt2s_hip.so; the host chooses crop starts, sorts text lengths and pads token ids.  A call copies a few
small tables to the device and reads nothing back.  Decoding files, file lists, shuffling and epochs stay host work of the caller.

Stated departure: the reference's TextMelLoader loads floats with librosa (resampling to the target rate) and then divides them by
max_wav_value a second time (utils/data_utils.py:18-20, 82).  TextMelBatch does what Mel2Samp does: int16 samples at the target
rate, divided once.  A corpus at another rate is brought to the target rate by PcmPool.resample / from_wav_files(resample=True) -
scipy.signal.resample_poly's filter, not librosa's.
"""
import random

import numpy as np
import torch

from . import _lib
from .audio import (LOUD_FLAG_NONFINITE, LOUD_FLAG_SHORT, LOUD_FLAG_SILENT, Limiter, Loudness, Resampler, SosFilter, TacotronSTFT,
                    Trimmer, _pcm16_gather, _to_device)

__all__ = ["PcmPool", "Mel2SampBatch", "TextMelBatch", "gather_width"]

T2SError = _lib.T2SError


def gather_width(longest, t_out, hop):
    """Row width T' of the gathered batch whose ragged mel is `mel_padded` itself: 1 + T' // hop == t_out and T' >= longest, for
    t_out >= 1 + longest // hop.  The smallest such width, rounded up to a multiple of 4 samples (16-byte rows) where that keeps the
    frame count."""
    if t_out < 1 + longest // hop:
        raise ValueError("t_out %d is below the %d frames of %d samples" % (t_out, 1 + longest // hop, longest))
    width = max(longest, (t_out - 1) * hop)
    up = -(-width // 4) * 4
    return up if up < t_out * hop else width


class PcmPool:
    """A corpus of int16 clips in HBM.  `clips`: a sequence of 1-D int16 numpy arrays or tensors (anything else raises T2SError:
    there is no silent cast).  `.pcm` is one int16 device tensor with all clips back to back, `.offsets` / `.lengths` host int64
    [n_clips], `.sampling_rate` the rate they were recorded at."""

    def __init__(self, clips, sampling_rate, device="cuda"):
        parts = []
        for i, c in enumerate(clips):
            if isinstance(c, np.ndarray):
                c = torch.from_numpy(np.ascontiguousarray(c)) if c.dtype == np.int16 and c.ndim == 1 else c
            if not torch.is_tensor(c) or c.dtype != torch.int16 or c.dim() != 1:
                raise T2SError("PcmPool: clip %d must be a 1-D int16 array or tensor, got %s %s" % (
                    i, getattr(c, "dtype", type(c).__name__), tuple(getattr(c, "shape", ()))))
            if c.numel() == 0:
                raise T2SError("PcmPool: clip %d is empty" % i)
            parts.append(c.detach())
        if not parts:
            raise T2SError("PcmPool: no clips")
        self.sampling_rate = sampling_rate
        self.lengths = torch.tensor([p.numel() for p in parts], dtype=torch.int64)
        self.offsets = torch.cumsum(self.lengths, 0) - self.lengths
        dev = torch.device(device)
        if dev.type != "cuda":
            raise T2SError("PcmPool: the pool lives in HBM (cuda); there is no CPU path")
        if any(p.is_cuda for p in parts):
            self.pcm = torch.cat([p.to(dev) for p in parts])
        else:
            self.pcm = torch.cat(parts).to(dev)             # one copy of the whole corpus

    def __len__(self):
        return self.lengths.numel()

    @classmethod
    def _of(cls, pcm, lengths, sampling_rate):
        """A pool around an int16 device tensor that already holds the clips back to back"""
        pool = cls.__new__(cls)
        pool.sampling_rate, pool.pcm = sampling_rate, pcm
        pool.lengths = lengths.to(torch.int64)
        pool.offsets = torch.cumsum(pool.lengths, 0) - pool.lengths
        return pool

    def resample(self, new_rate):
        """The pool at `new_rate`: every clip converted alone (Resampler: scipy.signal.resample_poly's filter, zero extension at the
        clip's own two ends, rounded to int16 with saturation), int16 to int16 in HBM in one launch.  Clip order and count are kept;
        clip i holds ceil(lengths[i] up / down) samples.  The same rate gives a copy."""
        if new_rate == self.sampling_rate:
            return self._of(self.pcm.clone(), self.lengths, new_rate)
        rs = Resampler(self.sampling_rate, new_rate, device=self.pcm.device)
        lengths = (self.lengths * rs.up + (rs.down - 1)) // rs.down
        pool = self._of(torch.empty(int(lengths.sum()), dtype=torch.int16, device=self.pcm.device), lengths, new_rate)
        rs._table(self.pcm, torch.stack([self.offsets, self.lengths, pool.offsets, pool.lengths], 1), pool.pcm, int(lengths.max()))
        return pool

    def rescale_trim(self, rescaling_max=None, top_db=None, frame_length=512, hop_length=128, pad_mode="reflect"):
        """The reference's corpus preparation between decoding and the mel (datasets/kss.py:68-74), as a new pool at the same rate
        and in the same clip order, int16 to int16 in HBM: every clip alone is scaled so that its largest sample becomes
        rescaling_max (`wav / abs(wav).max() * rescaling_max`, rounded to int16, ties to even) and cut to what
        librosa.effects.trim(wav, top_db, frame_length, hop_length) keeps (audio.Trimmer states the rule and pad_mode).  Either
        half is optional (None).  `pool.resample(rate).rescale_trim(0.999, 23)` is the reference's load, rescale, trim.

        With top_db the [n_clips, 2] cut points are read back once - the new offsets are their prefix sum on the host - and that is
        the only read.  A clip in which nothing is loud, or with pad_mode "reflect" one of at most frame_length // 2 samples, raises
        T2SError naming the clips; a pool holds no empty clip.  Stated departure: the reference keeps floats after rescaling, the
        pool rounds them to int16 (at most half an LSB); the cut points are decided on the source samples."""
        what = "PcmPool.rescale_trim"
        tr = Trimmer(frame_length, hop_length, top_db, pad_mode, rescaling_max)
        if top_db is None and rescaling_max is None:
            return self._of(self.pcm.clone(), self.lengths, self.sampling_rate)
        n, dev, chunk = len(self), self.pcm.device, 65535
        stats = torch.empty(n, 2, dtype=torch.float64, device=dev)
        frames = (1 + (self.lengths + 2 * tr.pad - tr.frame_length) // tr.hop_length).clamp(min=1)
        found = []
        for r0 in range(0, n, chunk):                       # 65535 rows a launch
            sl = slice(r0, min(n, r0 + chunk))
            e_off = torch.cumsum(frames[sl], 0) - frames[sl]
            table3 = _to_device(torch.stack([self.offsets[sl], self.lengths[sl], e_off], 1).contiguous(), dev)
            _, b = tr._stats_bounds(self.pcm, table3, table3.size(0), int(self.lengths[sl].max()), int(frames[sl].sum()), stats[sl])
            found.append(b)
        bounds_d, lengths = None, self.lengths
        if top_db is not None:
            bounds_d = found[0] if len(found) == 1 else torch.cat(found)
            bounds = bounds_d.cpu()                         # the one read: the new pool's offsets are a host prefix sum
            lengths = bounds[:, 1] - bounds[:, 0]
            short = torch.nonzero(self.lengths <= tr.pad).flatten().tolist() if pad_mode == "reflect" else []
            if short:
                raise T2SError("%s: clips %s have at most frame_length // 2 = %d samples (pad_mode 'reflect' needs more)"
                               % (what, short, tr.pad))
            empty = torch.nonzero(lengths <= 0).flatten().tolist()
            if empty:
                raise T2SError("%s: clips %s trim to nothing (no frame within %g dB of the loudest, or a clip of zeros)"
                               % (what, empty, tr.top_db))
        pool = self._of(torch.empty(int(lengths.sum()), dtype=torch.int16, device=dev), lengths, self.sampling_rate)
        table4 = _to_device(torch.stack([self.offsets, self.lengths, pool.offsets, pool.lengths], 1).contiguous(), dev)
        for r0 in range(0, n, chunk):
            sl = slice(r0, min(n, r0 + chunk))
            tr._gather(self.pcm, table4[sl], sl.stop - r0, None if bounds_d is None else bounds_d[sl], stats[sl], pool.pcm,
                       int(pool.lengths[sl].max()))
        return pool

    def _loudness(self, target_lufs, peak_limit):
        """(Loudness, stats float64 [n, 4], counts int32 [n, 4]) of every clip, 65535 rows a launch"""
        ld = Loudness(self.sampling_rate, target_lufs, peak_limit, device=self.pcm.device)
        n, dev, chunk = len(self), self.pcm.device, 65535
        stats = torch.empty(n, 4, dtype=torch.float64, device=dev)
        counts = torch.empty(n, 4, dtype=torch.int32, device=dev)
        table2 = _to_device(torch.stack([self.offsets, self.lengths], 1).contiguous(), dev)
        for r0 in range(0, n, chunk):
            sl = slice(r0, min(n, r0 + chunk))
            ld._measure(self.pcm, table2[sl], sl.stop - r0, int(self.lengths[sl].max()), stats[sl], counts[sl])
        return ld, stats, counts

    def loudness(self, target_lufs=-23.0):
        """BS.1770 / EBU R128 gated loudness of every clip (audio.Loudness states the rule; a sample counts as x / 32768):
        LoudnessReport(ms, lufs, peak, gain, blocks, flags), one entry per clip, on the device; `gain` is what brings the clip to
        target_lufs.  Nothing is read back."""
        _, stats, counts = self._loudness(target_lufs, None)
        return Loudness._report(stats, counts)

    def normalize_loudness(self, target_lufs=-23.0, peak_limit=32767 / 32768, allow_unmeasured=False):
        """Every clip brought to target_lufs, as a new pool at the same rate with the same lengths, int16 to int16 in HBM:
        rint(x gain), ties to even, saturated; the gain is cut so that the clip's largest sample stays within peak_limit (of full
        scale; None: no limit).  A clip shorter than 0.4 s, one with nothing above -70 LUFS and one that... cannot hold a non-finite
        sample, being int16: the first two have no loudness, and raise T2SError naming the clips - unless allow_unmeasured is set: then
        they are copied.  The flags are read back once (this is corpus preparation)."""
        ld, stats, counts = self._loudness(target_lufs, peak_limit)
        if not allow_unmeasured:
            flags = counts[:, 3].cpu()
            short = torch.nonzero(flags & LOUD_FLAG_SHORT).flatten().tolist()
            silent = torch.nonzero(flags & LOUD_FLAG_SILENT).flatten().tolist()
            bad = torch.nonzero(flags & LOUD_FLAG_NONFINITE).flatten().tolist()
            if short or silent or bad:
                raise T2SError("PcmPool.normalize_loudness: clips %s are shorter than 0.4 s, clips %s hold nothing above -70 LUFS, "
                               "clips %s a non-finite sample: they have no loudness (allow_unmeasured=True copies them)"
                               % (short, silent, bad))
        n, dev, chunk = len(self), self.pcm.device, 65535
        pool = self._of(torch.empty_like(self.pcm), self.lengths, self.sampling_rate)
        table4 = _to_device(torch.stack([self.offsets, self.lengths, pool.offsets, pool.lengths], 1).contiguous(), dev)
        for r0 in range(0, n, chunk):
            sl = slice(r0, min(n, r0 + chunk))
            ld._apply(self.pcm, table4[sl], sl.stop - r0, stats[sl], pool.pcm, int(self.lengths[sl].max()))
        return pool

    def _limiter(self, limiter, loudness, what):
        """(gains float64 [n] or None, stats float64 [n, 4], counts int32 [n, 2]) of every clip, 65535 rows a launch"""
        if not isinstance(limiter, Limiter):
            raise T2SError("%s: limiter must be an audio.Limiter, got a %s" % (what, type(limiter).__name__))
        if loudness is not None and not isinstance(loudness, Loudness):
            raise T2SError("%s: loudness must be None or an audio.Loudness, got a %s" % (what, type(loudness).__name__))
        for stage in (limiter, loudness):
            if stage is not None and stage.sampling_rate != self.sampling_rate:
                raise T2SError("%s: the %s is built for %d Hz, the pool holds %d Hz"
                               % (what, type(stage).__name__, stage.sampling_rate, self.sampling_rate))
        n, dev, chunk = len(self), self.pcm.device, 65535
        table2 = _to_device(torch.stack([self.offsets, self.lengths], 1).contiguous(), dev)
        gains = None
        if loudness is not None:
            lstats = torch.empty(n, 4, dtype=torch.float64, device=dev)
            lcounts = torch.empty(n, 4, dtype=torch.int32, device=dev)
            for r0 in range(0, n, chunk):
                sl = slice(r0, min(n, r0 + chunk))
                loudness._measure(self.pcm, table2[sl], sl.stop - r0, int(self.lengths[sl].max()), lstats[sl], lcounts[sl])
            gains = lstats[:, 3].contiguous()
        stats = torch.empty(n, 4, dtype=torch.float64, device=dev)
        counts = torch.empty(n, 2, dtype=torch.int32, device=dev)
        for r0 in range(0, n, chunk):
            sl = slice(r0, min(n, r0 + chunk))
            limiter._measure(self.pcm, table2[sl], sl.stop - r0, int(self.lengths[sl].max()), None if gains is None else gains[sl],
                             stats[sl], counts[sl])
        return gains, stats, counts

    def true_peak(self, limiter):
        """The true peak of every clip as `limiter` (an audio.Limiter at the pool's rate) meters it, a sample counting as
        x / 32768: LimiterReport(true_peak, sample_peak, min_gain, limited, flags), one entry per clip, on the device.  Nothing is
        read back."""
        _, stats, counts = self._limiter(limiter, None, "PcmPool.true_peak")
        return Limiter._report(stats, counts)

    def limit(self, limiter, loudness=None):
        """Every clip through `limiter` (audio.Limiter states the rule), as a new pool at the same rate with the same lengths in
        the same order, int16 to int16 in HBM: rint(32768 o), ties to even, saturated, so no code exceeds rint(32768 ceiling).  With
        `loudness` (an audio.Loudness at the pool's rate; build it with peak_limit=None) each clip is brought to its target first -
        the gain and the limiter in one pass; a clip that has no loudness (too short, silent) keeps gain 1.  Nothing is read back."""
        gains, _, counts = self._limiter(limiter, loudness, "PcmPool.limit")
        n, dev, chunk = len(self), self.pcm.device, 65535
        pool = self._of(torch.empty_like(self.pcm), self.lengths, self.sampling_rate)
        table4 = _to_device(torch.stack([self.offsets, self.lengths, pool.offsets, pool.lengths], 1).contiguous(), dev)
        for r0 in range(0, n, chunk):
            sl = slice(r0, min(n, r0 + chunk))
            limiter._apply(self.pcm, table4[sl], sl.stop - r0, None if gains is None else gains[sl], counts[sl], pool.pcm,
                           int(self.lengths[sl].max()))
        return pool

    def filter(self, filt):
        """Every clip through `filt` (an audio.SosFilter, which states the rule), as a new pool at the same rate with the same
        lengths in the same order, int16 to int16 in HBM: each clip alone from a zero state, filtered in the code domain in double
        and stored as rint(y), ties to even, saturated.  The new pool's `.clipped` and `.nonfinite` are int32 device tensors, one
        count per clip (the saturated samples; an int16 sample is always finite, so the second is zero).  A filter built with a
        sampling_rate other than the pool's is refused.  Nothing is read back."""
        what = "PcmPool.filter"
        if not isinstance(filt, SosFilter):
            raise T2SError("%s: filt must be an audio.SosFilter, got a %s" % (what, type(filt).__name__))
        if filt.sampling_rate is not None and filt.sampling_rate != self.sampling_rate:
            raise T2SError("%s: the filter was designed for %g Hz, the pool holds %g Hz" % (what, filt.sampling_rate, self.sampling_rate))
        n, dev, chunk = len(self), self.pcm.device, 65535
        pool = self._of(torch.empty_like(self.pcm), self.lengths, self.sampling_rate)
        table4 = _to_device(torch.stack([self.offsets, self.lengths, pool.offsets, pool.lengths], 1).contiguous(), dev)
        counts = torch.empty(n, 2, dtype=torch.int32, device=dev)
        for r0 in range(0, n, chunk):
            sl = slice(r0, min(n, r0 + chunk))
            filt._filter(self.pcm, table4[sl], sl.stop - r0, int(self.lengths[sl].max()), None, pool.pcm, int(self.lengths[sl].max()),
                         counts[sl])
        pool.nonfinite, pool.clipped = counts[:, 0], counts[:, 1]
        return pool

    @classmethod
    def from_wav_files(cls, paths, sampling_rate, device="cuda", resample=False):
        """Reads each file with scipy.io.wavfile.read.  A file that is not mono int16 is refused.  A file at another rate raises the
        reference's ValueError (waveglow/mel2samp.py:90-92) - unless `resample` is set: then files are uploaded as read, grouped by
        their rate, and each group is converted to sampling_rate on the device straight into its clips' places in the pool (one
        launch per source rate; PcmPool.resample's conversion, clip by clip), in the order of `paths`."""
        if not resample:
            return cls(cls.read_wav_files(paths, sampling_rate), sampling_rate, device)
        dev = torch.device(device)
        if dev.type != "cuda":
            raise T2SError("PcmPool: the pool lives in HBM (cuda); there is no CPU path")
        files = [cls._read_wav(path) for path in paths]
        if not files:
            raise T2SError("PcmPool: no clips")
        by_rate = {}
        for i, (rate, data) in enumerate(files):
            if data.size == 0:
                raise T2SError("PcmPool: clip %d is empty" % i)
            by_rate.setdefault(rate, []).append(i)
        converters = {rate: Resampler(rate, sampling_rate, device=dev) for rate in by_rate if rate != sampling_rate}
        lengths = torch.tensor([d.size if r == sampling_rate else converters[r].out_length(d.size) for r, d in files],
                               dtype=torch.int64)
        pool = cls._of(torch.empty(int(lengths.sum()), dtype=torch.int16, device=dev), lengths, sampling_rate)
        for rate, members in by_rate.items():
            if rate == sampling_rate:               # copied: one host-to-device copy per run of neighbouring files
                k = 0
                while k < len(members):
                    e = k
                    while e + 1 < len(members) and members[e + 1] == members[e] + 1:
                        e += 1
                    run = torch.from_numpy(np.concatenate([files[i][1] for i in members[k:e + 1]]))
                    first = int(pool.offsets[members[k]])
                    pool.pcm[first:first + run.numel()].copy_(run)
                    k = e + 1
                continue
            src_len = torch.tensor([files[i][1].size for i in members], dtype=torch.int64)
            src = torch.from_numpy(np.concatenate([files[i][1] for i in members])).to(dev)
            table = torch.stack([torch.cumsum(src_len, 0) - src_len, src_len, pool.offsets[members], lengths[members]], 1)
            converters[rate]._table(src, table, pool.pcm, int(lengths[members].max()))
        return pool

    @staticmethod
    def _read_wav(path, sampling_rate=None):
        """(rate, samples) of one file; a rate other than `sampling_rate` (where given) and a file that is not mono int16 are refused"""
        from scipy.io.wavfile import read
        rate, data = read(path)
        if sampling_rate is not None and rate != sampling_rate:
            raise ValueError("{} SR doesn't match target {} SR".format(rate, sampling_rate))
        if data.dtype != np.int16 or data.ndim != 1:
            raise T2SError("%s: expected mono int16 PCM, got %s with shape %s" % (path, data.dtype, data.shape))
        return rate, data

    @staticmethod
    def read_wav_files(paths, sampling_rate):
        """The host half of from_wav_files: the files' samples as a list of 1-D int16 arrays."""
        return [PcmPool._read_wav(path, sampling_rate)[1] for path in paths]

    def _indices(self, indices, what):
        idx = [int(i) for i in indices]
        if not idx:
            raise T2SError("%s: an empty batch" % what)
        for i in idx:
            if not 0 <= i < len(self):
                raise T2SError("%s: clip index %d outside the pool's %d clips" % (what, i, len(self)))
        return idx


def crop_starts(lengths, segment_length, rng):
    """Mel2Samp's crop per entry (waveglow/mel2samp.py:94-100): a clip of at least segment_length samples starts at
    rng.randint(0, len - segment_length), drawn in entry order; a shorter clip starts at 0 and consumes no draw."""
    return [rng.randint(0, n - segment_length) if n >= segment_length else 0 for n in lengths]


class Mel2SampBatch:
    """Mel2Samp's arguments with the pool in place of the file list (max_wav_value and n_mel_channels, constants of the reference's
    module, are keywords).  Called with clip indices it returns what a DataLoader over Mel2Samp hands `model((mel, audio))`:
    mel [B, n_mel_channels, 1 + segment_length // hop_length] and audio [B, segment_length], float32 in HBM.
    `rng`: a random.Random (default: seeded 1234, the reference's seed) that draws the crops; `starts` overrides the draws and
    `last_starts` keeps what was used.  The mel is the mel of the padded segment, as the reference computes it.  With
    max_wav_value >= 32768 every sample lies in [-1, 1] by construction, so mel_spectrogram's assertion and its read-back are
    skipped; any other value goes through mel_spectrogram."""

    def __init__(self, pool, segment_length, filter_length, hop_length, win_length, sampling_rate, mel_fmin, mel_fmax, rng=None,
                 max_wav_value=32768.0, n_mel_channels=80):
        if sampling_rate != pool.sampling_rate:
            raise ValueError("{} SR doesn't match target {} SR".format(pool.sampling_rate, sampling_rate))
        if segment_length <= filter_length // 2:
            raise T2SError("Mel2SampBatch: segment_length %d must exceed filter_length / 2" % segment_length)
        self.pool, self.segment_length, self.sampling_rate = pool, int(segment_length), sampling_rate
        self.max_wav_value = float(max_wav_value)
        self.rng = rng if rng is not None else random.Random(1234)
        self.stft = TacotronSTFT(filter_length=filter_length, hop_length=hop_length, win_length=win_length,
                                 n_mel_channels=n_mel_channels, sampling_rate=sampling_rate, mel_fmin=mel_fmin,
                                 mel_fmax=mel_fmax).to(pool.pcm.device)
        self.last_starts = None

    def __call__(self, indices, starts=None):
        what = "Mel2SampBatch"
        idx = self.pool._indices(indices, what)
        seg = self.segment_length
        lens = [int(self.pool.lengths[i]) for i in idx]
        if starts is None:
            starts = crop_starts(lens, seg, self.rng)
        else:
            starts = [int(s) for s in starts]
            if len(starts) != len(idx):
                raise T2SError("%s: %d starts for %d entries" % (what, len(starts), len(idx)))
            for s, n in zip(starts, lens):
                if not 0 <= s <= max(n - seg, 0):
                    raise T2SError("%s: start %d leaves no %d samples in a clip of %d" % (what, s, seg, n))
        self.last_starts = list(starts)
        table = torch.tensor([[int(self.pool.offsets[i]) + s, min(n - s, seg)] for i, s, n in zip(idx, starts, lens)],
                             dtype=torch.int64)
        audio = _pcm16_gather(self.pool.pcm, table, seg, self.max_wav_value)
        mel = self.stft._mel(audio)[0] if self.max_wav_value >= 32768.0 else self.stft.mel_spectrogram(audio)
        return mel, audio


class TextMelBatch:
    """TextMelLoader + TextMelCollate + Tacotron.parse_batch over a pool.  `sequences`: one list of symbol ids per clip
    (text.text_to_sequence); `speaker_ids`: one per clip (default 0).

    collate(indices) returns TextMelCollate's six results with the reference's shapes and dtypes - entries sorted by decreasing text
    length (torch.sort's order on ties), text_padded int64 zero padded, mel_padded [B, n_mel_channels, T_out] with zeros behind each
    entry (T_out: the most frames, rounded up to a multiple of n_frames_per_step), gate_padded 1 from each entry's last frame on,
    speaker_id float, output_lengths int64 - already in HBM, except input_lengths, which is on the host as the reference's is.
    Entry b's frames are, bit for bit, mel_spectrogram(clip / max_wav_value) of its clip alone.  __call__(indices) returns
    parse_batch's (x, y) of that batch, max_len a Python int.

    The clips are gathered in sorted order into rows just wide enough (gather_width) that the ragged mel is mel_padded itself.  A
    clip of at most filter_length / 2 samples is refused, as the mel refuses it alone.  With max_wav_value >= 32768 the [-1, 1]
    assertion holds by construction and nothing is read back; a smaller value goes through mel_spectrogram_batch and its assertion.

    speaker_id is in the order of `indices`, NOT in sorted order: that is what the reference's collate returns (it fills speaker_id
    before it walks the sorted ids, utils/data_utils.py:132-135), so with more than one speaker a row's id can belong to another
    row; pass indices already sorted by decreasing text length and every row has its own.

    Stated departure: the reference's TextMelLoader loads floats with librosa (resampling) and divides them by max_wav_value again
    (utils/data_utils.py:18-20, 82); this class does what Mel2Samp does - int16 at the target rate, divided once."""

    def __init__(self, pool, sequences, n_frames_per_step, filter_length, hop_length, win_length, n_mel_channels, sampling_rate,
                 mel_fmin, mel_fmax, max_wav_value=32768.0, speaker_ids=None):
        if sampling_rate != pool.sampling_rate:
            raise ValueError("{} SR doesn't match target {} SR".format(pool.sampling_rate, sampling_rate))
        if len(sequences) != len(pool):
            raise T2SError("TextMelBatch: %d sequences for %d clips" % (len(sequences), len(pool)))
        if speaker_ids is not None and len(speaker_ids) != len(pool):
            raise T2SError("TextMelBatch: %d speaker ids for %d clips" % (len(speaker_ids), len(pool)))
        if n_frames_per_step < 1:
            raise T2SError("TextMelBatch: n_frames_per_step must be at least 1")
        self.pool, self.n_frames_per_step, self.max_wav_value = pool, int(n_frames_per_step), float(max_wav_value)
        self.sequences = [torch.as_tensor(s, dtype=torch.int64).reshape(-1) for s in sequences]
        if any(s.numel() == 0 for s in self.sequences):
            raise T2SError("TextMelBatch: an empty sequence")
        self.speaker_ids = [0.0] * len(pool) if speaker_ids is None else [float(s) for s in speaker_ids]
        self.stft = TacotronSTFT(filter_length, hop_length, win_length, n_mel_channels, sampling_rate, mel_fmin,
                                 mel_fmax).to(pool.pcm.device)

    def collate(self, indices):
        what = "TextMelBatch"
        pool, dev = self.pool, self.pool.pcm.device
        idx = pool._indices(indices, what)
        hop, n_fft, step = self.stft.stft_fn.hop_length, self.stft.stft_fn.filter_length, self.n_frames_per_step
        input_lengths, order = torch.sort(torch.LongTensor([self.sequences[i].numel() for i in idx]), dim=0, descending=True)
        given, idx = idx, [idx[k] for k in order.tolist()]
        B = len(idx)
        lens = pool.lengths[idx]
        if int(lens.min()) <= n_fft // 2:
            raise T2SError("%s: clip %d has %d samples, the mel needs more than filter_length / 2 = %d" % (
                what, idx[int(lens.argmin())], int(lens.min()), n_fft // 2))
        t_out = 1 + int(lens.max()) // hop
        t_out = -(-t_out // step) * step
        width = gather_width(int(lens.max()), t_out, hop)
        text_padded = torch.zeros(B, int(input_lengths[0]), dtype=torch.int64)
        for k, i in enumerate(idx):
            text_padded[k, :self.sequences[i].numel()] = self.sequences[i]
        y = _pcm16_gather(pool.pcm, torch.stack([pool.offsets[idx], lens], 1), width, self.max_wav_value)
        if self.max_wav_value >= 32768.0:
            mel_padded, frames = self.stft._mel(y, lens)
        else:
            mel_padded, _ = self.stft.mel_spectrogram_batch(y, lens)
            frames = lens // hop + 1
        assert mel_padded.size(2) == t_out
        frames_d = _to_device(frames.to(torch.int32), dev)
        gate_padded = torch.empty(B, t_out, dtype=torch.float32, device=dev)
        _lib.call("t2s_gate_targets", _lib.ptr(frames_d), B, t_out, _lib.ptr(gate_padded), _lib.current_stream())
        speaker_id = _to_device(torch.tensor([self.speaker_ids[i] for i in given], dtype=torch.float32), dev)
        return _to_device(text_padded, dev), input_lengths, mel_padded, gate_padded, speaker_id, _to_device(frames, dev)

    def __call__(self, indices):
        text_padded, input_lengths, mel_padded, gate_padded, speaker_id, output_lengths = self.collate(indices)
        max_len = int(input_lengths[0])                  # sorted: the first is the longest; a host value, no .item() on the device
        x = (text_padded, _to_device(input_lengths, text_padded.device), mel_padded, max_len, speaker_id, output_lengths)
        return x, (mel_padded, gate_padded)
