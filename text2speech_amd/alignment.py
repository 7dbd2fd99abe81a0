"""The alignment check: does the attention path of a decoded utterance follow its text?

Tacotron-2 fails through its attention - it skips a symbol, goes back to one, stalls, or never reaches the end.  ``alignment_report``
looks at the alignments that ``Tacotron.inference`` / ``inference_batch`` / ``forward`` return, on the device (csrc/align.hip;
include/t2s_hip.h states the arithmetic): per frame the symbol it attends to, per entry the largest forward and backward step, the
longest stall, the last symbol reached, the frames each symbol got (its duration) and the mean attention peak - and the flag bits that
an ``AlignmentCheck``'s thresholds make of them.  ``synthesize_long(check=, max_attempts=)`` decodes a flagged chunk again under
``attempt_seeds``: the prenet dropout is live in eval mode, so another seed is another attention path.  ``AlignmentStream`` is the same
report pushed piece by piece while an utterance is still decoded (csrc/align.hip): the watchdog of
``synthesize_stream(control=StreamControl(check=))``, which ends a stream whose attention fails instead of speaking it out."""
import collections

import torch

from . import _lib, sampling
from .longform import _MASK, mix

__all__ = ["AlignmentCheck", "AlignmentReport", "alignment_report", "AlignmentStream", "attempt_seeds", "FLAG_NAMES", "STAT_NAMES", "LIVE"]

TRUNCATED, SKIP, BACK, STALL, UNFINISHED, DIFFUSE, NONFINITE, EMPTY = 1, 2, 4, 8, 16, 32, 64, 128
FLAG_NAMES = {TRUNCATED: "TRUNCATED", SKIP: "SKIP", BACK: "BACK", STALL: "STALL", UNFINISHED: "UNFINISHED", DIFFUSE: "DIFFUSE",
              NONFINITE: "NONFINITE", EMPTY: "EMPTY"}
STAT_NAMES = ("frames", "symbols", "max_skip", "max_back", "longest_stall", "last_pos", "covered", "bad_rows")
ATTEMPT_STEP = 0xD1342543DE82EF95      # odd: attempt k of seed s draws from mix(s + k ATTEMPT_STEP) >> 1

_KINDS = {torch.float32: 1, torch.float16: 2}

AlignmentReport = collections.namedtuple("AlignmentReport", "flags stats focus durations path")


class AlignmentCheck:
    """The thresholds of the alignment check; a negative integer (or ``min_focus <= 0``) switches its flag off.

      skip_max    SKIP        the path moves forward by more than this many symbols from one frame to the next
      back_max    BACK        ... backward by more than this many
      stall_max   STALL       more than this many consecutive frames on one symbol
      end_slack   UNFINISHED  the last frame attends more than this many symbols before the last one
      min_focus   DIFFUSE     the mean attention peak over the frames is not at least this
      max_frames  TRUNCATED   the entry has at least this many frames; None: the decoder's max_decoder_steps where a model is at hand
                              (``synthesize_long``), else off
    NONFINITE (a frame's weights hold a NaN or an infinity) and EMPTY (no frame) have no threshold.

    The defaults - 4, 2, 80, 2, 0.3 - are guesses at what a decoder trained on sentence-length clips does when it reads well (a
    step of one symbol a frame or less, a pause of under half a second at hop 256 and 44 800 Hz, a peak well above 1 / symbols); no
    trained checkpoint has been measured here.  Tune them on yours: ``alignment_report``'s stats are the quantities they bound."""
    __slots__ = ("skip_max", "back_max", "stall_max", "end_slack", "min_focus", "max_frames")

    def __init__(self, skip_max=4, back_max=2, stall_max=80, end_slack=2, min_focus=0.3, max_frames=None):
        for name, v in (("skip_max", skip_max), ("back_max", back_max), ("stall_max", stall_max), ("end_slack", end_slack),
                        ("max_frames", max_frames)):
            if name == "max_frames" and v is None:
                continue
            if isinstance(v, bool) or not isinstance(v, int) or not -2 ** 31 <= v < 2 ** 31:
                raise ValueError("AlignmentCheck: %s must be an int32 integer%s, got %r"
                                 % (name, " or None" if name == "max_frames" else "", v))
        if isinstance(min_focus, bool) or not isinstance(min_focus, (int, float)) or min_focus != min_focus:
            raise ValueError("AlignmentCheck: min_focus must be a number, got %r" % (min_focus,))
        self.skip_max, self.back_max, self.stall_max, self.end_slack = skip_max, back_max, stall_max, end_slack
        self.min_focus, self.max_frames = float(min_focus), max_frames

    def thresholds(self, max_frames=None):
        """(max_frames, skip_max, back_max, stall_max, end_slack, min_focus) as the entry point takes them; ``max_frames`` is used
        where the check's own is None (0: off)"""
        own = self.max_frames if self.max_frames is not None else (0 if max_frames is None else int(max_frames))
        return own, self.skip_max, self.back_max, self.stall_max, self.end_slack, self.min_focus

    def with_max_frames(self, max_frames):
        """this check, with ``max_frames`` in the place of a None"""
        if self.max_frames is not None:
            return self
        return AlignmentCheck(self.skip_max, self.back_max, self.stall_max, self.end_slack, self.min_focus, int(max_frames))

    def __repr__(self):
        return "AlignmentCheck(%s)" % ", ".join("%s=%r" % (n, getattr(self, n)) for n in self.__slots__)


def attempt_seeds(seed, k):
    """The seed of attempt ``k`` of an utterance whose own seed is ``seed``: attempt 0 is the seed itself, attempt k >= 1 is
    ``mix(seed + k C) >> 1`` in wrapping uint64 arithmetic with C = 0xD1342543DE82EF95 (odd, so k C never repeats below 2^64) and
    ``longform.mix`` - a Python int in [0, 2^63).  A sequence of seeds gives the list of their attempt-k seeds."""
    if isinstance(k, bool) or not isinstance(k, int) or k < 0:
        raise ValueError("attempt_seeds: k must be an integer >= 0, got %r" % (k,))
    if isinstance(seed, (list, tuple)):
        return [attempt_seeds(s, k) for s in seed]
    seed = sampling.check_seed(seed, "attempt_seeds: seed")
    return seed if k == 0 else mix((seed + k * ATTEMPT_STEP) & _MASK) >> 1


def _lengths(lengths, B, dev, what):
    """a [B] tensor of lengths for the kernels: int32 on the device.  A device tensor is used as it is (an int64 one through a
    cast to int32 - a copy, its values are not looked at); host values go up through page-locked memory without a wait."""
    from .audio import _to_device
    if lengths is None:
        return None
    T2SError = _lib.T2SError
    try:
        lens = torch.as_tensor(lengths)
    except (TypeError, ValueError, RuntimeError) as e:
        raise T2SError("alignment_report: %s must be a tensor or a sequence of integers (%s)" % (what, e))
    if lens.dtype not in (torch.int32, torch.int64) and not (lens.device.type == "cpu" and lens.dtype in (torch.int16, torch.uint8,
                                                                                                          torch.int8)):
        raise T2SError("alignment_report: %s must be int32 or int64, got %s" % (what, lens.dtype))
    if lens.dim() != 1 or lens.numel() != B:
        raise T2SError("alignment_report: %s has shape %s, the batch holds %d entries" % (what, tuple(lens.shape), B))
    lens = lens.detach()
    if lens.is_cuda:
        if lens.device != dev:
            raise T2SError("alignment_report: %s live on %s, the alignments on %s" % (what, lens.device, dev))
        return lens.to(torch.int32).contiguous()
    return _to_device(lens.to(torch.int64).clamp(-1, 2 ** 31 - 1).to(torch.int32), dev)


def alignment_report(alignments, input_lengths=None, output_lengths=None, check=None):
    """Where every frame attends and whether that path is the text, computed on the device.

    ``alignments`` [B, N, T_in] float32 or float16 in HBM: what ``Tacotron.inference`` (B = 1, no lengths needed),
    ``inference_batch`` or ``forward`` return, of a float or a ``.half()`` model.  A view whose last dimension is dense and whose
    rows and entries do not overlap (strides [>= N ld, ld >= T_in, 1]) is read where it is; any other is copied first.
    ``input_lengths`` / ``output_lengths`` [B]: the symbols and the frames of every entry (None: T_in, N).  A device tensor (int32,
    or int64 as ``inference_batch`` returns its output lengths) is used as it is; host values go up through page-locked memory.
    Either way the kernels clamp them to [1, T_in] and [0, N].  ``check``: an ``AlignmentCheck`` (None: the default thresholds; its
    ``max_frames=None`` is off here, where no decoder is at hand).

    Returns AlignmentReport(flags, stats, focus, durations, path), all on the device:
      flags      int32 [B]: 0 is a pass; bits TRUNCATED 1, SKIP 2, BACK 4, STALL 8, UNFINISHED 16, DIFFUSE 32, NONFINITE 64, EMPTY 128
      stats      int32 [B, 8]: frames, symbols, max_skip, max_back, longest_stall, last_pos, covered, bad_rows (STAT_NAMES)
      focus      float64 [B]: the mean attention peak; an entry's bits do not depend on its batch
      durations  int32 [B, T_in]: the frames that attend to each symbol - what word timing needs
      path       int32 [B, N]: the symbol every frame attends to, -1 behind an entry's last frame

    Two launches and a memset on the caller's current stream; nothing is read back and no arithmetic runs on the values outside the
    two kernels."""
    T2SError = _lib.T2SError
    if not (torch.is_tensor(alignments) and alignments.is_cuda):
        raise T2SError("alignment_report: expected alignments in HBM (cuda); there is no CPU path")
    if alignments.dim() != 3 or alignments.numel() == 0:
        raise T2SError("alignment_report: alignments must be [B, N, T_in] and hold values, got %s" % (tuple(alignments.shape),))
    A = alignments.detach()
    if A.dtype not in _KINDS:
        raise T2SError("alignment_report: expected float32 or float16, got %s (there is no silent cast)" % A.dtype)
    if check is None:
        check = AlignmentCheck()
    elif not isinstance(check, AlignmentCheck):
        raise T2SError("alignment_report: check must be an AlignmentCheck, got a %s" % type(check).__name__)
    B, N, T = A.shape
    if B * N > 2 ** 31 - 1:
        raise T2SError("alignment_report: %d x %d frames, the most is 2^31 - 1" % (B, N))
    dev = A.device
    in_len = _lengths(input_lengths, B, dev, "input_lengths")
    out_len = _lengths(output_lengths, B, dev, "output_lengths")
    ld_row = A.stride(1) if N > 1 else T
    ld_entry = A.stride(0) if B > 1 else N * ld_row
    if A.stride(2) != 1 or ld_row < T or ld_entry < N * ld_row:
        A = A.contiguous()
        ld_row, ld_entry = T, N * T
    with torch.cuda.device(dev):
        path = torch.empty(B, N, dtype=torch.int32, device=dev)
        peak = torch.empty(B, N, dtype=torch.float32, device=dev)
        bad = torch.empty(B, N, dtype=torch.uint8, device=dev)
        stats = torch.empty(B, 8, dtype=torch.int32, device=dev)
        focus = torch.empty(B, dtype=torch.float64, device=dev)
        dur = torch.empty(B, T, dtype=torch.int32, device=dev)
        flags = torch.empty(B, dtype=torch.int32, device=dev)
        p, st = _lib.ptr, _lib.current_stream()
        _lib.call("t2s_align_rows", p(A), _KINDS[A.dtype], B, N, T, ld_row, ld_entry, p(in_len), p(out_len), p(path), p(peak), p(bad),
                  st)
        _lib.call("t2s_align_stats", p(path), p(peak), p(bad), B, N, T, p(in_len), p(out_len), *check.thresholds(), p(stats),
                  p(focus), p(dur), p(flags), st)
    return AlignmentReport(flags, stats, focus, dur, path)


LIVE = SKIP | BACK | STALL | NONFINITE      # the bits a stream's prefix can already decide; the others wait for its last push


class AlignmentStream:
    """``alignment_report`` pushed piece by piece while the utterance is still decoded (csrc/align.hip): the watchdog of a stream.

    ``check`` an ``AlignmentCheck`` (None: the defaults; its ``max_frames=None`` is ``capacity``), ``n_symbols`` the columns of an
    alignment row, ``capacity`` the most frames there can be (the decoder's max_decoder_steps), ``B`` entries that grow together,
    ``input_lengths`` their symbols (None: n_symbols).

    ``push(align_piece [B, n, n_symbols], last)`` - float32 or float16, what ``Tacotron.inference_stream`` yields as ``piece[3]`` -
    enqueues the window kernels and an asynchronous copy of flags and stats into page-locked memory, with an event behind it: no
    wait, and nothing is read on the host.  After every push the buffers on the device hold what ``alignment_report`` gives for the
    frames seen so far, bit for bit (the running maxima, the counts and the 256 partial sums of the peaks are carried in HBM); the
    flags of a push not flagged ``last`` carry only the ``LIVE`` bits - SKIP, BACK, STALL, NONFINITE - and those of the last push
    all eight.  A stall counts while it is still open, so it is seen while it happens.

    ``report()``: an ``AlignmentReport`` of the prefix, on the device (copies; ``path`` holds the frames seen).  ``poll()``: the host
    ``(flags int32 [B], stats int32 [B, 8])`` of the latest push whose copy has completed, or None; ``wait()``: the same for the
    latest push, after ``event.synchronize()``.  ``path`` int32 [B, capacity] is the persistent buffer a ``WarpStream`` reads."""
    SLOTS = 4

    def __init__(self, check, n_symbols, capacity, device, B=1, input_lengths=None):
        who = "AlignmentStream"
        T2SError = _lib.T2SError
        if check is None:
            check = AlignmentCheck()
        elif not isinstance(check, AlignmentCheck):
            raise T2SError("%s: check must be an AlignmentCheck, got a %s" % (who, type(check).__name__))
        for name, v in (("n_symbols", n_symbols), ("capacity", capacity), ("B", B)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError("%s: %s must be an integer >= 1, got %r" % (who, name, v))
        if capacity > 2 ** 30 or B * capacity > 2 ** 31 - 1:
            raise T2SError("%s: %d x %d frames, the most is 2^31 - 1 (2^30 an entry)" % (who, B, capacity))
        dev = torch.device(device)
        if dev.type != "cuda":
            raise T2SError("%s: the stream lives in HBM (cuda); there is no CPU path" % who)
        self.check, self.n_symbols, self.capacity, self.device, self.B = check, n_symbols, capacity, dev, B
        self._thr = check.thresholds(capacity)
        self._in_len = _lengths(input_lengths, B, dev, "input_lengths")
        nbytes = _lib.load().t2s_align_window_state()
        with torch.cuda.device(dev):
            self.path = torch.empty(B, capacity, dtype=torch.int32, device=dev)
            self._peak = torch.empty(B, capacity, dtype=torch.float32, device=dev)
            self._bad = torch.empty(B, capacity, dtype=torch.uint8, device=dev)
            self._state = torch.empty(B, nbytes // 8, dtype=torch.int64, device=dev)
            self._out = torch.empty(B, 9, dtype=torch.int32, device=dev).view(-1)       # stats [B, 8], then flags [B]
            self._focus = torch.empty(B, dtype=torch.float64, device=dev)
            self._dur = torch.empty(B, n_symbols, dtype=torch.int32, device=dev)
        self._host = [torch.empty(B * 9, dtype=torch.int32).pin_memory() for _ in range(self.SLOTS)]
        self._events = [None] * self.SLOTS
        self.frames = 0
        self.pushes = 0
        self.ended = False
        self._order = _lib.StreamOrder()

    def push(self, align_piece, last):
        who = "AlignmentStream.push"
        T2SError = _lib.T2SError
        if self.ended:
            raise T2SError("%s: a piece arrived behind the one flagged last" % who)
        if not (torch.is_tensor(align_piece) and align_piece.is_cuda and align_piece.device == self.device):
            raise T2SError("%s: expected alignments on %s" % (who, self.device))
        A = align_piece.detach()
        if A.dim() != 3 or A.size(0) != self.B or A.size(2) != self.n_symbols:
            raise T2SError("%s: a piece must be [%d, n, %d], got %s" % (who, self.B, self.n_symbols, tuple(A.shape)))
        if A.dtype not in _KINDS:
            raise T2SError("%s: expected float32 or float16, got %s (there is no silent cast)" % (who, A.dtype))
        m, T, B = A.size(1), self.n_symbols, self.B
        n0, n = self.frames, self.frames + m
        if n > self.capacity:
            raise T2SError("%s: %d frames, the stream was made for %d" % (who, n, self.capacity))
        ld_row = A.stride(1) if m > 1 else T
        ld_entry = A.stride(0) if B > 1 else m * ld_row
        if m and (A.stride(2) != 1 or ld_row < T or ld_entry < m * ld_row):
            A = A.contiguous()
            ld_row, ld_entry = T, m * T
        cur = self._order.enter(self.device)
        if self._order.switched:
            _lib.record_stream((self.path, self._peak, self._bad, self._state, self._out, self._focus, self._dur, self._in_len), cur)
        p = _lib.ptr
        slot = self.pushes % self.SLOTS
        with torch.cuda.device(self.device):
            _lib.call("t2s_align_window", p(A) if m else None, _KINDS[A.dtype], B, self.capacity, T, n0, n, int(bool(last)), ld_row,
                      ld_entry, p(self._in_len), *self._thr, p(self.path), p(self._peak), p(self._bad), p(self._state),
                      p(self._out), p(self._focus), p(self._dur), p(self._out[8 * B:]), _lib.current_stream())
            self._host[slot].copy_(self._out, non_blocking=True)
            ev = self._events[slot]
            if ev is None:
                ev = self._events[slot] = torch.cuda.Event()
            ev.record(cur)
        self.frames = n
        self.pushes += 1
        self.ended = bool(last)

    def _read(self, slot):
        h = self._host[slot]
        return h[8 * self.B:].clone(), h[:8 * self.B].view(self.B, 8).clone()

    def poll(self):
        """host (flags, stats) of the latest push whose copy has completed; None where there is none yet"""
        for k in range(self.pushes - 1, max(-1, self.pushes - 1 - self.SLOTS), -1):
            if self._events[k % self.SLOTS].query():
                return self._read(k % self.SLOTS)
        return None

    def wait(self):
        """host (flags, stats) of the latest push, after waiting for its copy"""
        if not self.pushes:
            return None
        slot = (self.pushes - 1) % self.SLOTS
        self._events[slot].synchronize()
        return self._read(slot)

    def report(self):
        if not self.pushes:
            raise _lib.T2SError("AlignmentStream.report: nothing has been pushed yet")
        B, n = self.B, self.frames
        return AlignmentReport(self._out[8 * B:].clone(), self._out[:8 * B].view(B, 8).clone(), self._focus.clone(), self._dur.clone(),
                               self.path[:, :n].clone())
