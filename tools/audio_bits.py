#!/usr/bin/env python3
"""The bits of the PCM kernels that share csrc/pcm_rows.h, csrc/resample_tap.h and csrc/limit_tile.h, as one sha256 per output buffer.

    python tools/audio_bits.py > a.txt                                         # this tree's library
    T2S_LIB_PATH=build/parent/libt2s_hip.so python tools/audio_bits.py > b.txt # another build of it, in a fresh process
    diff a.txt b.txt

Calls t2s_resample_batch, t2s_resample_table, t2s_limit_measure + t2s_limit_apply, t2s_resample_window, t2s_limit_window,
t2s_loud_apply and t2s_trim_gather on seeded inputs and prints `<case> <buffer> <sha256>` lines (the return code where it is not 0).
It asserts nothing about a library alone: two libraries compute the same iff their outputs are the same text.  The shapes are the
smallest that reach every branch: rows of 3 tiles + 40 samples, 1 and 3 rows, int16 / f32 / f16 sources, int16 destinations,
ratios 15/14, 5/28 and 2/1, (look-ahead, oversampling) (0, 1), (1, 2), (67, 4), (1024, 4), no gain and a gain of 8 (the first tile
of a row is quiet enough to stay below the ceiling either way: it takes the skip), one row that is not limited, one that holds a
NaN, and pieces of 0, 1, C - 1, C + 1, 1023 and 1025 samples in front of the rest."""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from text2speech_amd import _lib, audio  # noqa: E402

DEV = "cuda:0"
TILE = 1024
N_ROW = 3 * TILE + 40
HW, CEILING = 10, float(np.float32(10.0 ** (-1.0 / 20.0)))
RATIOS = ((15, 14), (5, 28), (2, 1))
LIMITERS = ((0, 1), (1, 2), (67, 4), (1024, 4))
KINDS = {"int16": (0, torch.int16), "f32": (1, torch.float32), "f16": (2, torch.float16)}
FILL = 12345.0


def emit(case, name, t, rc=0):
    t = t.detach().contiguous().cpu()
    h = hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()
    print("%s %s %s%s" % (case, name, h, "" if rc == 0 else " rc=%d" % rc), flush=True)


def rows_f64(B, n, seed, nan_row=None):
    """quiet over the first tile and a half, loud behind it; row 1 of a batch quiet throughout (never limited)"""
    g = np.random.RandomState(seed)
    x = g.randn(B, n) * 0.3
    x[:, :TILE + TILE // 2] *= 0.03
    if B > 1:
        x[1] *= 0.003
    x = np.clip(x, -0.999, 0.999)
    if nan_row is not None:
        x[nan_row, 2 * TILE + 7] = np.nan
    return x


def to_kind(x, kind):
    if kind == "int16":
        return torch.from_numpy(np.rint(np.nan_to_num(x) * 32767.0).astype(np.int16))
    return torch.from_numpy(x).to(KINDS[kind][1])


def pool(rows, kind, pad):
    """rows [B, n] -> (flat device tensor, row stride): `pad` elements of 1e4 / 9999 between the rows and behind the last"""
    B, n = rows.shape
    ld = n + pad
    flat = torch.full((B * ld,), 9999 if kind == "int16" else 1e4, dtype=KINDS[kind][1])
    flat.view(B, ld)[:, :n] = to_kind(rows, kind)
    return flat.to(DEV), ld


def i64(rows):
    return torch.tensor(rows, dtype=torch.int64, device=DEV)


def filled(n, dtype):
    return torch.full((max(1, n),), FILL if dtype.is_floating_point else 12345, dtype=dtype, device=DEV)


def resample_cases(lib, st):
    for up, down in RATIOS:
        u, d, h = audio.resample_filter(down, up)
        assert (u, d) == (up, down)
        hd = torch.from_numpy(h).to(DEV)
        n = -(-N_ROW * down // up)
        n_out = -(-n * up // down)
        for B in (1, 3):
            x = rows_f64(B, n, 100 * up + down + B)
            lens = [n - 37 * b for b in range(B)]
            for kind in ("f32", "f16"):
                case = "resample_batch %d/%d B%d %s" % (up, down, B, kind)
                src, ldx = pool(x, kind, 1)
                out, ol = filled(B * n_out, torch.float32), filled(B, torch.int32)
                ld = torch.tensor(lens, dtype=torch.int32, device=DEV)
                rc = lib.t2s_resample_batch(src.data_ptr(), int(kind == "f16"), B, n, ldx, ld.data_ptr(), hd.data_ptr(), h.size, up, down,
                                            out.data_ptr(), n_out, n_out, ol.data_ptr(), st)
                emit(case, "out", out, rc)
                emit(case, "out_lengths", ol)
            for kind in KINDS:
                for dk, ddt in ((0, torch.int16), (1, torch.float32)):
                    case = "resample_table %d/%d B%d %s->%s" % (up, down, B, kind, "int16" if dk == 0 else "f32")
                    src, ldx = pool(x, kind, 3)
                    cap = n_out + 9                             # zeros behind a row's end, up to its cap
                    table = i64([(b * ldx, lens[b], b * (cap + 5), cap) for b in range(B)])
                    out, ol = filled(B * (cap + 5), ddt), filled(B, torch.int32)
                    rc = lib.t2s_resample_table(src.data_ptr(), KINDS[kind][0], src.numel(), table.data_ptr(), B, hd.data_ptr(), h.size, up,
                                                down, out.data_ptr(), dk, out.numel(), cap, ol.data_ptr(), st)
                    emit(case, "out", out, rc)
                    emit(case, "out_lengths", ol)


def limit_tables(L, os_):
    return torch.from_numpy(audio.resample_filter(1, os_, HW, 5.0)[2]).to(DEV), torch.from_numpy(audio.limiter_window(L)).to(DEV)


def gains_of(g, B):
    return None if g is None else torch.tensor([g * (1 + 0.25 * b) for b in range(B)], dtype=torch.float64, device=DEV)


def limit_cases(lib, st):
    n = N_ROW
    for L, os_ in LIMITERS:
        h, w = limit_tables(L, os_)
        for B in (1, 3):
            for kind in KINDS:
                x = rows_f64(B, n, 7 * L + os_ + B, nan_row=2 if B == 3 and kind != "int16" else None)
                for g in (None, 8.0):
                    case = "limit L%d os%d B%d %s gain %s" % (L, os_, B, kind, g)
                    src, ldx = pool(x, kind, 1)
                    gd = gains_of(g, B)
                    gp = gd.data_ptr() if gd is not None else None
                    lens = [n - 411 * b for b in range(B)]
                    cap = n + 6
                    table2 = i64([(b * ldx, lens[b]) for b in range(B)])
                    table4 = i64([(b * ldx, lens[b], b * cap, cap) for b in range(B)])
                    need = lib.t2s_limit_scratch(B, n)
                    scratch = torch.zeros(need, dtype=torch.float64, device=DEV)
                    stats, counts = filled(4 * B, torch.float64), filled(2 * B, torch.int32)
                    ddt, dk = (torch.int16, 0) if kind == "int16" else (torch.float32, 1)
                    out, ol = filled(B * cap, ddt), filled(B, torch.int32)
                    rc = lib.t2s_limit_measure(src.data_ptr(), KINDS[kind][0], src.numel(), table2.data_ptr(), B, n, gp, h.data_ptr(), h.numel(),
                                               os_, HW, w.data_ptr(), L, CEILING, scratch.data_ptr(), need, stats.data_ptr(), counts.data_ptr(),
                                               st)
                    emit(case, "scratch", scratch, rc)
                    emit(case, "stats", stats)
                    emit(case, "counts", counts)
                    rc = lib.t2s_limit_apply(src.data_ptr(), KINDS[kind][0], src.numel(), table4.data_ptr(), B, gp, h.data_ptr(), h.numel(), os_,
                                             HW, w.data_ptr(), L, CEILING, counts.data_ptr(), out.data_ptr(), dk, out.numel(), cap,
                                             ol.data_ptr(), st)
                    emit(case, "out", out, rc)
                    emit(case, "out_lengths", ol)


def pieces_of(n, C):
    """piece lengths 0, 1, C - 1, C + 1, 1023, 1025 (each cut to what the row still holds), then the rest"""
    cuts, left = [], n
    for c in (0, 1, C - 1, C + 1, 1023, 1025):
        cuts.append(min(c, left))
        left -= cuts[-1]
    return cuts + [left]


def stream(case, B, x, kind, Cn, call, end, state=None):
    """the windows of one stream: outputs concatenated, the last carry, the state"""
    carry = [torch.full((B * Cn,), float("nan"), dtype=torch.float32, device=DEV) for _ in range(2)]
    pos = done = 0
    cuts = pieces_of(x.shape[1], Cn)
    outs, rcs = [], 0
    for q, c in enumerate(cuts):
        final = int(q == len(cuts) - 1)
        piece, ldp = pool(x[:, pos:pos + c], kind, 2) if c else (None, 0)
        m = end(pos + c, done, final) - done
        out = filled(B * m, torch.float32)
        rc = call(carry[q % 2].data_ptr(), carry[1 - q % 2].data_ptr(), piece.data_ptr() if c else None, int(kind == "f16"), B, c, ldp, pos,
                  done, final, out.data_ptr() if m else None, m, m)
        rcs = rcs or rc
        outs.append(out[:B * m].view(B, m))
        pos += c
        done += m
    emit(case, "out", torch.cat(outs, 1), rcs)
    emit(case, "carry", carry[len(cuts) % 2])
    if state is not None:
        emit(case, "state", state)


def window_cases(lib, st):
    for up, down in RATIOS:
        _, _, h = audio.resample_filter(down, up)
        hd = torch.from_numpy(h).to(DEV)
        n = -(-N_ROW * down // up)
        Cn = lib.t2s_resample_window_carry(h.size, up)
        for B in (1, 3):
            x = rows_f64(B, n, 100 * up + down + B)
            for kind in ("f32", "f16"):
                stream("resample_window %d/%d B%d %s" % (up, down, B, kind), B, x, kind, Cn,
                       lambda ci, co, p, half, B_, n_, ldp, K0, M0, fin, o, cap, ldo: lib.t2s_resample_window(
                           ci, co, p, half, B_, n_, ldp, K0, M0, fin, hd.data_ptr(), h.size, up, down, o, cap, ldo, st),
                       lambda K1, M0, fin: lib.t2s_resample_window_end(K1, M0, h.size, up, down, fin))
    for L, os_ in LIMITERS:
        h, w = limit_tables(L, os_)
        Cn = lib.t2s_limit_window_carry(L, HW)
        for B in (1, 3):
            for kind in ("f32", "f16"):
                x = rows_f64(B, N_ROW, 7 * L + os_ + B, nan_row=2 if B == 3 else None)
                for g in (None, 8.0):
                    gd = gains_of(g, B)
                    gp = gd.data_ptr() if gd is not None else None
                    state = torch.tensor([0, 0, 0x3FF0000000000000, 0, 0] * B, dtype=torch.int64, device=DEV)
                    stream("limit_window L%d os%d B%d %s gain %s" % (L, os_, B, kind, g), B, x, kind, Cn,
                           lambda ci, co, p, half, B_, n_, ldp, N0, O0, fin, o, cap, ldo: lib.t2s_limit_window(
                               ci, co, p, half, B_, n_, ldp, N0, O0, fin, gp, h.data_ptr(), h.numel(), os_, HW, w.data_ptr(), L, CEILING, o,
                               cap, ldo, state.data_ptr(), st),
                           lambda N1, O0, fin: lib.t2s_limit_window_end(N1, O0, L, HW, fin), state)


def row_cases(lib, st):
    """the loudness apply and the trim gather: a gain per row (1 copies), a kept range per row, zeros up to the cap"""
    n, B = N_ROW, 3
    x = rows_f64(B, n, 5)
    lens = [n - 411 * b for b in range(B)]
    cap = n + 6
    for kind in KINDS:
        src, ldx = pool(x, kind, 1)
        ddt, dk = (torch.int16, 0) if kind == "int16" else (torch.float32, 1)
        table = i64([(b * ldx, lens[b], b * cap, cap) for b in range(B)])
        stats = torch.tensor([[0.0, 0.0, 0.0, gn] for gn in (1.0, 0.37, 8.0)], dtype=torch.float64, device=DEV)
        out, ol = filled(B * cap, ddt), filled(B, torch.int32)
        rc = lib.t2s_loud_apply(src.data_ptr(), KINDS[kind][0], src.numel(), table.data_ptr(), B, stats.data_ptr(), out.data_ptr(), dk,
                                out.numel(), cap, ol.data_ptr(), st)
        emit("loud_apply %s" % kind, "out", out, rc)
        emit("loud_apply %s" % kind, "out_lengths", ol)
        bounds = i64([(0, lens[0]), (513, 2 * TILE + 1), (TILE, lens[2] + 50)])
        peaks = torch.tensor([[0.9 * (32767.0 if kind == "int16" else 1.0), 0.0]] * B, dtype=torch.float64, device=DEV)
        for with_stats in (False, True):
            out, ol = filled(B * cap, ddt), filled(B, torch.int32)
            rc = lib.t2s_trim_gather(src.data_ptr(), KINDS[kind][0], src.numel(), table.data_ptr(), B, bounds.data_ptr(),
                                     peaks.data_ptr() if with_stats else None, 0.999, 0.0, out.data_ptr(), dk, out.numel(), cap,
                                     ol.data_ptr(), st)
            case = "trim_gather %s %s" % (kind, "rescaled" if with_stats else "copied")
            emit(case, "out", out, rc)
            emit(case, "out_lengths", ol)


def main():
    assert torch.cuda.is_available(), "needs the device"
    lib = _lib.load()
    assert lib.t2s_limit_tile() == TILE == lib.t2s_resample_tile()
    st = _lib.current_stream()
    for cases in (resample_cases, limit_cases, window_cases, row_cases):
        cases(lib, st)
        torch.cuda.synchronize()


if __name__ == "__main__":
    main()
