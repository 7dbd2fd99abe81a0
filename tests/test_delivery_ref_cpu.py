"""The chunked delivery chain of tests/delivery_ref.py against the whole-row restatement, bit for bit, on the CPU: every ratio, every
limiter setting, the piece-length cycle {0, 1, C - 1, C, C + 1, 1023, 1025, 7} with C the carry of the stage the pieces enter; the
running state against the whole row's statistics; the muting rule; the G.711 tables over all 65 536 codes against audioop; and the
carry / M1 / O1 formulas as host arithmetic, against their definitions and against the library's host-only entry points."""
import numpy as np
import pytest

import delivery_ref as D
import limiter_ref as LR
import resample_ref as RR
from text2speech_amd import _lib

C_DB = LR.ceiling(LR.CEILING_DB)


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _row_and_cuts(C, seed, L, flush=False, kind="float32"):
    n = sum(D.piece_cycle(C)) + 300
    cuts = D.cuts_for(n, C, flush)
    return D.row(n, seed, kind, peaks=D.peaks_at(n, cuts, L)), cuts


@pytest.mark.parametrize("limiter", D.LIMITERS)
@pytest.mark.parametrize("ratio", D.RATIOS)
def test_the_chunked_chain_is_the_whole_chain(ratio, limiter):
    up, down, h = RR.filter_ref(*ratio)
    C = D.resample_carry(h.size, up)
    x, cuts = _row_and_cuts(C, 11 * up + down + limiter[0], limiter[0], flush=(up + limiter[1]) % 2 == 0)
    for g in (1.0, 8.0):
        whole, stats, counts = D.chain_whole(x, ratio, limiter, C_DB, g)
        outs, state = D.chain_chunked(x, cuts, ratio, limiter, C_DB, g)
        assert _same_bits(np.concatenate(outs), whole)
        assert (state["tp"], state["sp"], state["smin"]) == stats[:3] and (state["count"], state["flags"]) == counts
        assert np.abs(whole).max() <= C_DB
    assert counts[0] > 0, "the row was limited: the test is about something"


@pytest.mark.parametrize("ratio", D.RATIOS)
def test_the_chunked_resampler_alone(ratio):
    up, down, h = RR.filter_ref(*ratio)
    C = D.resample_carry(h.size, up)
    for flush, kind in ((False, "float16"), (True, "float32")):
        x, cuts = _row_and_cuts(C, 5 + up, 0, flush, kind)
        outs, _ = D.chain_chunked(x, cuts, ratio, None, C_DB)
        assert _same_bits(np.concatenate(outs), D.chain_whole(x, ratio, None, C_DB)[0])
        assert sum(o.size for o in outs) == RR.out_length(x.size, up, down)


@pytest.mark.parametrize("limiter", D.LIMITERS)
def test_the_chunked_limiter_alone_with_pieces_around_its_own_carry(limiter):
    L, os = limiter
    C = D.limit_carry(L)
    for flush, kind, g in ((False, "float32", 1.0), (True, "float16", 3.0)):
        x, cuts = _row_and_cuts(C, 77 + L, L, flush, kind)
        whole, stats, counts = D.chain_whole(x, None, limiter, C_DB, g)
        outs, state = D.chain_chunked(x, cuts, None, limiter, C_DB, g)
        assert _same_bits(np.concatenate(outs), whole)
        assert (state["tp"], state["sp"], state["smin"]) == stats[:3] and (state["count"], state["flags"]) == counts
        assert counts[0] > 0
        # what a not-final window holds back is the reach, never more
        held = np.cumsum(cuts)[:-1] - np.cumsum([o.size for o in outs])[:-1]
        assert held.max() <= D.limit_reach(L)


def test_one_sample_pieces():
    for ratio, limiter in (((5, 14), (16, 4)), ((2, 1), (1, 2))):
        x = D.row(90, 3, peaks=(0, 40, 89))
        outs, _ = D.chain_chunked(x, [1] * 90, ratio, limiter, C_DB, 2.0)
        assert _same_bits(np.concatenate(outs), D.chain_whole(x, ratio, limiter, C_DB, 2.0)[0])


def test_a_sample_that_is_not_finite_mutes_and_is_flagged():
    L, os = 16, 4
    x = D.row(700, 9, peaks=(100, 500))
    x[300], x[420] = np.nan, np.inf
    outs, state = D.chain_chunked(x, [250, 60, 200, 190], None, (L, os), C_DB)
    out = np.concatenate(outs)
    assert np.isfinite(out).all() and state["flags"] & LR.FLAG_NONFINITE and state["tp"] == np.inf and state["smin"] == 0.0
    assert out[300] == 0 and out[420] == 0 and np.abs(out).max() <= C_DB
    reach = D.limit_reach(L)
    ref = LR.limit(np.where(np.isfinite(x), x, 0).astype(np.float32), C_DB, L, os).out
    assert _same_bits(out[:300 - reach], ref[:300 - reach]) and _same_bits(out[420 + reach + 1:], ref[420 + reach + 1:])


def test_the_carry_and_end_formulas():
    lib = _lib.load()
    for up, down in D.RATIOS + ((1, 512), (512, 1), (160, 147)):
        n_taps = 2 * 10 * max(up, down) + 1
        half = n_taps // 2
        C = D.resample_carry(n_taps, up)
        assert lib.t2s_resample_window_carry(n_taps, up) == C == -(-n_taps // up)
        M0 = 0
        for K1 in list(range(0, 40)) + [half // up, half // up + 1, 1000, 1023, 44800, 10 ** 9]:
            M1 = D.resample_end(K1, M0, n_taps, up, down, False)
            assert lib.t2s_resample_window_end(K1, M0, n_taps, up, down, 0) == M1
            # the definition: output m may go out once the sample under its last tap, floor((half + m down) / up), is below K1
            assert M1 == M0 or (half + (M1 - 1) * down) // up < K1
            assert (half + M1 * down) // up >= K1, "... and output M1 may not"
            # ... and its first tap's sample lies inside the carry of the window before
            assert (M1 * down - half) / up >= K1 - C
            fin = D.resample_end(K1, M0, n_taps, up, down, True)
            assert lib.t2s_resample_window_end(K1, M0, n_taps, up, down, 1) == fin == max(M0, RR.out_length(K1, up, down))
            M0 = M1
    for L, hw in ((0, 10), (1, 10), (16, 10), (67, 10), (1024, 32), (0, 1)):
        reach = 2 * L + hw
        assert lib.t2s_limit_window_carry(L, hw) == D.limit_carry(L, hw) == 2 * reach
        for N1, O0 in ((0, 0), (5, 0), (reach, 0), (reach + 1, 0), (5000, 4000), (5000, 4990), (2 ** 33, 2 ** 33 - 9000)):
            for final in (0, 1):
                assert lib.t2s_limit_window_end(N1, O0, L, hw, final) == D.limit_end(N1, O0, L, hw, final)
    assert lib.t2s_resample_window_carry(2, 1) == -1 and lib.t2s_limit_window_carry(1025, 10) == -1 and lib.t2s_limit_window_carry(5, 33) == -1
    assert lib.t2s_resample_window_end(-1, 0, 41, 2, 1, 0) == -1 and lib.t2s_limit_window_end(-1, 0, 5, 10, 0) == -1


def test_g711_over_every_code_against_audioop():
    audioop = pytest.importorskip("audioop")
    codes = np.arange(-32768, 32768, dtype=np.int64).astype(np.int16)
    raw = codes.astype("<i2").tobytes()
    assert D.ulaw(codes).tobytes() == audioop.lin2ulaw(raw, 2)
    assert D.alaw(codes).tobytes() == audioop.lin2alaw(raw, 2)
    # round trip: the decoded byte is within the quantisation step of its segment
    back = np.frombuffer(audioop.ulaw2lin(D.ulaw(codes).tobytes(), 2), "<i2").astype(np.int64)
    assert np.abs(back - np.clip(codes.astype(np.int64), -32635, 32635)).max() <= 1024


def test_pcm16_restates_the_truncation():
    x = np.array([0.0, 1.0, -1.0, 0.5, -0.5, 0.99999, 3.0, -3.0, np.nan, 1 / 32768, -1 / 32768, 1.5 / 32768, -1.5 / 32768], np.float32)
    assert D.pcm16(x).tolist() == [0, 32767, -32768, 16384, -16384, 32767, 32767, -32768, 0, 1, -1, 1, -1]
