"""Biquad cascades restated in float64 (numpy + scipy.signal.sosfilt): the reference of csrc/sosfilt.hip and the cases its tests
use.  Three forms:
  sequential      scipy.signal.sosfilt on the substituted input - the reference every accuracy bar is measured from;
  parallel        the kernel's order - segments from zero, a Hillis-Steele scan over 256 lanes with the host table's maps, the
                  segments again from the state in front, tiles chained by the table's tile map - vectorised over the lanes.  numpy
                  has no fused multiply-add, so this is the kernel's ORDER, not its bits: E = max |parallel - sequential| is what
                  the reordering costs in double, measured on the CPU between two references and never from the device;
  ParallelStream  the chunked form: the state at the start of the current tile and the samples since then, recomputed per piece.
tests/test_filter_ref_cpu.py pins this file; the GPU tests compare the device with `sequential` under the bar `bar()` states."""
import math

import numpy as np
from scipy.signal import butter, sosfilt

SEGMENT, LANES = 16, 256        # t2s_sos_segment(), t2s_sos_tile() / it: the GPU tests assert that the library says the same
TILE = SEGMENT * LANES
MAX_SECTIONS = 8
TAB_POW, TAB_TILE, TAB_DOUBLES = 40, 296, 552
N_ACC = 17161                   # the accuracy rows: four tiles and 777 samples


# ---- the filters --------------------------------------------------------------------------------------------------------------
def peaking(f0, Q, gain_db, fs):
    """one peaking section of the audio-EQ cookbook, a0 normalised to exactly 1"""
    A = 10.0 ** (gain_db / 40.0)
    w0 = 2.0 * math.pi * f0 / fs
    alpha = math.sin(w0) / (2.0 * Q)
    a0 = 1.0 + alpha / A
    return np.array([[(1.0 + alpha * A) / a0, -2.0 * math.cos(w0) / a0, (1.0 - alpha * A) / a0, 1.0, -2.0 * math.cos(w0) / a0,
                      (1.0 - alpha / A) / a0]])


def _butter(order, cut, kind, fs):
    return np.ascontiguousarray(butter(order, cut, kind, fs=fs, output="sos"), dtype=np.float64)


# name -> (sos, the second term of the bar as a multiple of 2^-24 max|ref| must stay below 1/4: True for the accuracy cases)
ACCURACY_CASES = {
    "deemphasis_0.97": np.array([[1.0, 0.0, 0.0, 1.0, -0.97, 0.0]]),
    "preemphasis_0.97": np.array([[1.0, -0.97, 0.0, 1.0, 0.0, 0.0]]),
    "highpass_80_o4_44800": _butter(4, 80.0, "highpass", 44800.0),
    "highpass_20_o2_44800": _butter(2, 20.0, "highpass", 44800.0),
    "telephone_300_3400_o4_8000": _butter(4, [300.0, 3400.0], "bandpass", 8000.0),
    "lowpass_3400_o8_44800": _butter(8, 3400.0, "lowpass", 44800.0),
    "peaking_q8_1000_44800": peaking(1000.0, 8.0, 6.0, 44800.0),
}
LOOSE_INT16 = ("highpass_20_o2_44800",)         # the one accuracy case whose int16 output may differ by a code near a half-integer
# the kind of filter this form cannot hold to a float32 ulp (direct-form double arithmetic itself disagrees with itself by 6e-9 at
# unit level): in the bit-equality tests only
HIGHPASS_5 = _butter(2, 5.0, "highpass", 48000.0)
BIT_CASES = dict(ACCURACY_CASES, highpass_5_o2_48000=HIGHPASS_5)


def sections_case(n):
    """a well-conditioned cascade of exactly n sections, 1 <= n <= 8: telephone-band sections and peaking sections in turn"""
    tel = _butter(4, [300.0, 3400.0], "bandpass", 8000.0)
    rows = [tel[j % 4] if j % 2 == 0 else peaking(500.0 + 300.0 * j, 2.0, 3.0 - j, 16000.0)[0] for j in range(n)]
    return np.array(rows)


def impulse_l1(sos, n=1 << 16):
    """G: the l1 norm of the cascade's impulse response (its first n samples: the tails of these filters are far below a rounding)"""
    d = np.zeros(n)
    d[0] = 1.0
    return float(np.sum(np.abs(sosfilt(sos, d))))


# ---- the inputs ---------------------------------------------------------------------------------------------------------------
def input_rows(n=N_ACC):
    """name -> samples as the device receives them (float32 or int16), seeded.  The int16 codes are multiples of 4 (14-bit material
    in a 16-bit container): 0.97 x is then never a half-integer (388 m = 50 mod 100 has no solution), whereas with arbitrary codes
    one pre-emphasis output in a hundred is an exact tie, which no bar measured on the references can tell from a near-tie."""
    rng = np.random.RandomState(20251)
    t = np.arange(n)
    noise = (0.3 * rng.randn(n)).astype(np.float32)
    mix = (0.05 + 0.4 * np.sin(2.0 * math.pi * 0.011 * t) + 0.2 * np.sin(2.0 * math.pi * 0.23 * t + 1.0) + 0.05 * rng.randn(n)).astype(
        np.float32)
    codes = np.clip(4.0 * np.rint(1500.0 * rng.randn(n)), -32768, 32764).astype(np.int16)
    return {"noise_f32": noise, "mix_f32": mix, "codes_i16": codes}


def substitute(x, gain=1.0):
    """the samples as they enter the filter: widened to double, times the gain, +0 where that is not finite -> (x64, nonfinite)"""
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.asarray(x).astype(np.float64) * float(gain)
    bad = ~np.isfinite(v)
    v[bad] = 0.0
    return v, int(bad.sum())


def round16(y):
    """pcm_round16 of csrc/pcm_rows.h -> (int16 codes, clipped)"""
    q = np.rint(np.asarray(y, dtype=np.float64))
    clipped = int(np.sum((q > 32767.0) | (q < -32768.0)))
    return np.clip(q, -32768.0, 32767.0).astype(np.int16), clipped


# ---- the three forms ----------------------------------------------------------------------------------------------------------
def sequential(sos, x, gain=1.0):
    """-> (y float64, nonfinite): scipy.signal.sosfilt on the substituted input"""
    v, bad = substitute(x, gain)
    if v.size == 0:
        return v, bad
    return sosfilt(np.asarray(sos, dtype=np.float64), v), bad


def _tile(tab, n, xt, start):
    """one tile of TILE samples (zeros behind the row) from the cascade state `start` [2n] -> (outputs [TILE], the scanned end
    state of lane 255, section by section [2n])"""
    X = xt.reshape(LANES, SEGMENT).copy()
    end = np.zeros(2 * n)
    for j in range(n):
        b0, b1, b2, a1, a2 = tab[5 * j:5 * j + 5]
        u0, u1 = np.zeros(LANES), np.zeros(LANES)
        u0[0], u1[0] = start[2 * j], start[2 * j + 1]
        for i in range(SEGMENT):
            x = X[:, i]
            y = b0 * x + u0
            u0 = (b1 * x + u1) - a1 * y
            u1 = b2 * x - a2 * y
        for k in range(8):
            d = 1 << k
            P = tab[TAB_POW + 32 * j + 4 * k:TAB_POW + 32 * j + 4 * k + 4]
            q0, q1 = u0[:-d].copy(), u1[:-d].copy()
            u0[d:] = (u0[d:] + P[0] * q0) + P[1] * q1
            u1[d:] = (u1[d:] + P[2] * q0) + P[3] * q1
        end[2 * j], end[2 * j + 1] = u0[-1], u1[-1]
        t0 = np.concatenate([[start[2 * j]], u0[:-1]])
        t1 = np.concatenate([[start[2 * j + 1]], u1[:-1]])
        for i in range(SEGMENT):
            x = X[:, i]
            y = b0 * x + t0
            t0 = (b1 * x + t1) - a1 * y
            t1 = b2 * x - a2 * y
            X[:, i] = y
    return X.reshape(-1), end


def parallel_from(tab, n, v, start):
    """the kernel's order over the substituted samples v from the cascade state `start` at a tile's first sample -> (y float64, the
    state at the start of tile len(v) // TILE)"""
    d = 2 * n
    P = tab[TAB_TILE:TAB_TILE + d * d].reshape(d, d)
    c = np.array(start, dtype=np.float64)
    zero = np.zeros(d)
    y = np.empty(v.size)
    for q in range(-(-v.size // TILE)):
        seg = v[q * TILE:(q + 1) * TILE]
        xt = np.zeros(TILE)
        xt[:seg.size] = seg
        y[q * TILE:q * TILE + seg.size] = _tile(tab, n, xt, c)[0][:seg.size]
        if seg.size == TILE:
            e = _tile(tab, n, xt, zero)[1]
            nxt = np.empty(d)
            for i in range(d):
                acc = e[i]
                for j in range(d):
                    acc = acc + P[i, j] * c[j]
                nxt[i] = acc
            c = nxt
    return y, c


def parallel(sos, tab, x, gain=1.0):
    """-> (y float64, nonfinite): the whole row in the kernel's order; `tab` is audio.sos_table(sos, SEGMENT, LANES)"""
    v, bad = substitute(x, gain)
    n = np.asarray(sos).shape[0]
    return parallel_from(tab, n, v, np.zeros(2 * n))[0], bad


class ParallelStream:
    """the chunked form: push(piece) -> the piece's outputs (float64); `nonfinite` runs"""

    def __init__(self, sos, tab, gain=1.0):
        self.n = np.asarray(sos).shape[0]
        self.tab, self.gain = tab, gain
        self.state = np.zeros(2 * self.n)
        self.held = np.zeros(0, dtype=np.float32)              # the row's samples since the start of its current tile, as f32
        self.nonfinite = 0

    def push(self, piece):
        piece = np.asarray(piece)
        assert piece.dtype in (np.float32, np.float16)
        self.nonfinite += substitute(piece, self.gain)[1]
        buf = np.concatenate([self.held, piece.astype(np.float32)])
        y, state = parallel_from(self.tab, self.n, substitute(buf, self.gain)[0], self.state)
        out = y[self.held.size:]
        self.held = buf[buf.size // TILE * TILE:]
        self.state = state
        return out


# ---- the bar ------------------------------------------------------------------------------------------------------------------
def second_term(E, G, x_max):
    return 16.0 * max(E, 2.0 ** -50 * G * x_max)


def bar(ref, E, G, x_max):
    """what a float32 output may differ from the sequential float64 `ref` by, per sample"""
    return 2.0 ** -24 * np.abs(ref) + second_term(E, G, x_max)


def int16_exempt(ref, term):
    """the samples whose `ref` lies within `term` of a half-integer: there the int16 output may differ by one code"""
    frac = np.abs(ref - np.floor(ref) - 0.5)
    return frac <= term


_measured = {}


def measure(case, row):
    """(sos, x, ref float64, E, G, the bar's second term) of an accuracy case on an input row, computed once: E is the largest
    difference between the parallel-order and the sequential float64 forms - two references, no device"""
    key = (case, row)
    if key not in _measured:
        from text2speech_amd.audio import sos_table
        sos, x = BIT_CASES[case], input_rows()[row]
        ref, _ = sequential(sos, x)
        par, _ = parallel(sos, sos_table(sos, SEGMENT, LANES), x)
        E, G = float(np.max(np.abs(par - ref))), impulse_l1(sos)
        _measured[key] = (sos, x, ref, E, G, second_term(E, G, float(np.max(np.abs(x.astype(np.float64))))))
    return _measured[key]


# ---- cuts ---------------------------------------------------------------------------------------------------------------------
def cut_patterns(L, seed=0):
    """name -> piece lengths that sum to L: the cuts every chunked test walks"""
    rng = np.random.RandomState(1000 + seed)
    pats = {"one": [L]}
    if 0 < L <= 300:
        pats["ones"] = [1] * L
    for name, k in (("S-1", SEGMENT - 1), ("S", SEGMENT), ("S+1", SEGMENT + 1), ("T-1", TILE - 1), ("T", TILE), ("T+1", TILE + 1)):
        if L > k:
            pats[name] = [k, min(3, L - k)] + ([L - k - 3] if L - k > 3 else [])
    if L > 2 * TILE + 100:
        pats["long"] = [5, 2 * TILE + 61, L - 2 * TILE - 66]
    if L >= 2:
        cuts = np.sort(rng.randint(0, L + 1, size=9))
        cuts[4] = cuts[3]                                       # an empty piece inside
        edges = np.concatenate([[0], cuts, [L]])
        pats["random"] = [int(b - a) for a, b in zip(edges[:-1], edges[1:])] + [0]       # and an empty final flush
    for v in pats.values():
        assert sum(v) == L and min(v) >= 0
    return pats


# ---- T2S_EINVAL -----------------------------------------------------------------------------------------------------------------
# Parameter names in ABI order; a change maps a name to a value, to None (NULL) or to ("+", bytes): the pointer moved by that much.
FILTER_PARAMS = ("src src_kind src_len table n_rows max_count gains tab n_sections scratch scratch_len dst dst_kind dst_len max_out "
                 "counts stream").split()
WINDOW_PARAMS = "carry_in carry_out piece is_half B n ldp N0 gains tab n_sections scratch scratch_len out ldo counts stream".split()


def filter_refusals():
    """(label, changes) pairs, each breaking one rule of t2s_sos_filter for a valid f32 -> f32 call"""
    v = [("NULL " + p, {p: None}) for p in ("src", "table", "tab", "scratch", "dst", "counts")]
    v += [("misaligned " + p, {p: ("+", 4)}) for p in ("table", "gains", "tab", "scratch")]
    v += [("misaligned counts", {"counts": ("+", 2)}), ("misaligned src", {"src": ("+", 2)}), ("misaligned dst", {"dst": ("+", 2)})]
    v += [("src_kind = -1", dict(src_kind=-1)), ("src_kind = 3", dict(src_kind=3)), ("dst_kind = 2", dict(dst_kind=2)),
          ("dst_kind = -1", dict(dst_kind=-1)), ("f32 -> int16", dict(dst_kind=0)), ("src_len = 0", dict(src_len=0)),
          ("dst_len = 0", dict(dst_len=0)), ("n_rows = 0", dict(n_rows=0)), ("n_rows = 65536", dict(n_rows=65536)),
          ("max_count = 0", dict(max_count=0)), ("max_count = 2^31", dict(max_count=2 ** 31)), ("max_out = 0", dict(max_out=0)),
          ("max_out > 2^40", dict(max_out=2 ** 40 + 1)), ("n_sections = 0", dict(n_sections=0)),
          ("n_sections = 9", dict(n_sections=MAX_SECTIONS + 1)), ("scratch_len one short", dict(scratch_len=("-", 1))),
          ("dst inside src", dict(dst="src"))]
    return v


def window_refusals():
    """... of t2s_sos_window for a valid f32 call with n > 0"""
    v = [("NULL " + p, {p: None}) for p in ("carry_in", "carry_out", "piece", "tab", "scratch", "out", "counts")]
    v += [("misaligned " + p, {p: ("+", 4)}) for p in ("carry_in", "carry_out", "gains", "tab", "scratch")]
    v += [("misaligned counts", {"counts": ("+", 2)}), ("misaligned piece", {"piece": ("+", 2)}), ("misaligned out", {"out": ("+", 2)})]
    v += [("is_half = 2", dict(is_half=2)), ("is_half = -1", dict(is_half=-1)), ("B = 0", dict(B=0)), ("B = 65536", dict(B=65536)),
          ("n = -1", dict(n=-1)), ("n = 2^31", dict(n=2 ** 31)), ("ldp < n", dict(ldp=("-", 1))), ("ldo < n", dict(ldo=("-", 1))),
          ("N0 = -1", dict(N0=-1)), ("N0 > 2^40", dict(N0=2 ** 40 + 1)), ("n_sections = 0", dict(n_sections=0)),
          ("n_sections = 9", dict(n_sections=MAX_SECTIONS + 1)), ("scratch_len one short", dict(scratch_len=("-", 1))),
          ("carry_out is carry_in", dict(carry_out="carry_in"))]
    return v


def apply_changes(base, changes):
    """base: name -> int (pointers as integers) -> the argument dict with `changes` applied"""
    out = dict(base)
    for k, c in changes.items():
        if c is None:
            out[k] = None
        elif isinstance(c, tuple):
            out[k] = base[k] + c[1] if c[0] == "+" else base[k] - c[1]
        elif isinstance(c, str):
            out[k] = base[c]
        else:
            out[k] = c
    return out
